"""Expected outputs of per-link depth thresholds (include/rtuf.h, PER-LINK DEPTH THRESHOLDS) from the CPU oracle's debug planes,
for the tests and scripts/link_thresholds_rate.py.  The oracle's `prim` is the winning source triangle of every pixel, numbered
over the draw list it was given (-2: the background quad, -1: no fragment); a drawn pixel is compared with that triangle's
draw -> link -> threshold, the background quad's with the global one, and the compare is the shader's in numpy float32 with
the host's shade_num / shade_off order of operations (dilation_check.shade).  The oracle itself is not changed (numpy only)."""
import numpy as np

from bench_support.dilation_check import drawn_z, shade


def prim_thresholds(draw_thr, draw_ntris):
    """Threshold of every oracle primitive id: draw d owns the next draw_ntris[d] ids."""
    return np.repeat(np.asarray(draw_thr, np.float32), np.asarray(draw_ntris, np.int64)).astype(np.float32)


def pixel_thresholds(prim, draw_thr, draw_ntris, global_thr):
    """[H,W] float32 threshold of every pixel: its winner's link's, the global one where the background quad won (prim -2)
    or nothing was drawn (prim -1: not compared at all)."""
    table = prim_thresholds(draw_thr, draw_ntris)
    out = np.full(prim.shape, np.float32(global_thr), np.float32)
    drawn = prim >= 0
    out[drawn] = table[prim[drawn]]
    return out


def expected_planes(zwin, prim, sensor, draw_thr, draw_ntris, global_thr, z_near, z_far, replace):
    """(masked f32, mask u8 0 / 255) of one plane: the GL clear colour (0, 0) where nothing was drawn."""
    t = pixel_thresholds(prim, draw_thr, draw_ntris, global_thr)
    return shade(drawn_z(zwin, prim), np.asarray(sensor, np.float32), z_near, z_far, t, replace)


def link_values(n_links, global_thr, per_model=None, link_base=None):
    """Threshold of every link of a context: global_thr where a model inherits; per_model {model index: [one per link]}
    with link_base[model] the model's first link (the order rtuf_add_model / rtuf_add_link made them)."""
    v = np.full(n_links, np.float32(global_thr), np.float32)
    for m, t in (per_model or {}).items():
        v[link_base[m]:link_base[m] + len(t)] = np.asarray(t, np.float32)
    return v


def workload_draws(wl, link_thr):
    """(threshold, triangle count) of every draw of bench_support Workload.oracle_draws(s), in that order (the same for every
    stream); link_thr indexes the context's links as wl.load_into creates them."""
    thr, ntris, g = [], [], 0
    for links in wl.models:
        for draws in links:
            for d in draws:
                thr.append(np.float32(link_thr[g]))
                ntris.append(len(d.tris))
            g += 1
    return thr, ntris


def workload_link_base(wl):
    """First link of every model of a Workload in the context wl.load_into fills."""
    base, out = 0, []
    for links in wl.models:
        out.append(base)
        base += len(links)
    return out


def share_draws(share, s, link_thr):
    """(threshold, triangle count) of every draw of configs.RankShare.oracle_frame(k, s), in that order; link_thr indexes the
    context's links (share.link_base of each model id + the link's index)."""
    g = share.group_of(s)
    thr, ntris = [], []
    for m, links in zip(g.model_ids, g.variants[0].models):
        for li, draws in enumerate(links):
            for d in draws:
                thr.append(np.float32(link_thr[share.link_base[m] + li]))
                ntris.append(len(d.tris))
    return thr, ntris
