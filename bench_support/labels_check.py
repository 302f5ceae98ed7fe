"""Expected link label planes (include/rtuf.h, LINK LABELS) from the CPU oracle's debug output, for the tests and
scripts/labels_rate.py.  The oracle's `prim` is the winning source triangle of every pixel, numbered over the draw list it
was given (-2: the background quad, -1: no fragment); the label plane is that triangle's draw -> link -> label, 0 for -1
and -2 (numpy only)."""
import numpy as np


def prim_labels(draw_labels, draw_ntris):
    """Label of every oracle primitive id: draw d owns the next draw_ntris[d] ids."""
    return np.repeat(np.asarray(draw_labels, np.int64), np.asarray(draw_ntris, np.int64)).astype(np.uint16)


def expected_labels(prim, draw_labels, draw_ntris):
    """[H,W] uint16 label plane from the oracle's prim plane and the label of every draw it was given."""
    table = prim_labels(draw_labels, draw_ntris)
    out = np.zeros(prim.shape, np.uint16)
    drawn = prim >= 0
    out[drawn] = table[prim[drawn]]
    return out


def default_link_labels(n_links):
    """Default labels of a context's links, numbered over all models in creation order: 1 + global link index."""
    return np.arange(1, n_links + 1, dtype=np.int64)


def workload_draws(wl, link_label=None):
    """(label, triangle count) of every draw of bench_support Workload.oracle_draws(s), in that order (the same for every
    stream); link_label indexes the context's links as wl.load_into creates them (default labels if None)."""
    n_links = sum(len(links) for links in wl.models)
    link_label = default_link_labels(n_links) if link_label is None else np.asarray(link_label)
    labels, ntris, g = [], [], 0
    for links in wl.models:
        for draws in links:
            for d in draws:
                labels.append(int(link_label[g]))
                ntris.append(len(d.tris))
            g += 1
    return labels, ntris


def share_draws(share, s, link_label=None):
    """(label, triangle count) of every draw of configs.RankShare.oracle_frame(k, s), in that order; link_label indexes the
    context's links (share.link_base of each model id + the link's index; default labels if None)."""
    link_label = default_link_labels(share.n_links_total) if link_label is None else np.asarray(link_label)
    g = share.group_of(s)
    labels, ntris = [], []
    for m, links in zip(g.model_ids, g.variants[0].models):
        for li, draws in enumerate(links):
            for d in draws:
                labels.append(int(link_label[share.link_base[m] + li]))
                ntris.append(len(d.tris))
    return labels, ntris
