/*
 * rtuf.h -- C ABI of the MI355X-native realtime URDF depth self-filter.
 *
 * This is the drop-in boundary for the hot path of blodow/realtime_urdf_filter:
 *   RealtimeURDFFilter::filter() -> textureBufferFromDepthBuffer() -> render()
 *   -> URDFRenderer::render() -> Renderable*::render() -> urdf_filter.{vert,frag}
 *   -> glGetTexImage read-back.
 * Every entry point cites the reference interface it replaces (paths relative to
 * the reference checkout).  The reference has no C ABI of its own -- its boundary
 * is the C++ class surface of include/realtime_urdf_filter/urdf_filter.h:51-143 and
 * urdf_renderer.h:45-73 -- so these are the calls a C++ facade (include/
 * realtime_urdf_filter_amd/urdf_filter.hpp), a ROS adapter or a ctypes/cgo/JNI stub
 * binds (INTEGRATION.md shows the bindings).
 *
 * Conventions: plain pointers and sizes only; every function returns an int status
 * (RTUF_OK = 0, negative = error) and never throws; rtuf_last_error() returns the
 * message of the last failure on that context (or of rtuf_create when ctx == NULL).
 * The caller owns every host buffer; the library owns device memory.  One context is
 * bound to one GPU and used from one host thread at a time; several contexts (one per
 * GPU) may run concurrently.  All matrices are OpenGL style: 16 values, column-major.
 *
 * There is NO CPU fallback: without a visible gfx950 device (hipDeviceProp_t::gcnArchName) rtuf_create()
 * fails with RTUF_ERR_NO_DEVICE.
 */
#ifndef RTUF_H_
#define RTUF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTUF_ABI_VERSION 6

typedef struct rtuf_context rtuf_context;

enum {
  RTUF_OK = 0,
  RTUF_ERR_INVALID = -1,      /* bad argument / call order                      */
  RTUF_ERR_NO_DEVICE = -2,    /* no usable HIP device (no CPU fallback exists)  */
  RTUF_ERR_HIP = -3,          /* HIP runtime error, see rtuf_last_error         */
  RTUF_ERR_OOM = -4,          /* host or device allocation failed               */
  RTUF_ERR_CAPACITY = -5,     /* a per-tile bin overflowed even after regrowth  */
  RTUF_ERR_STATE = -6         /* models not finalised / frame not ready         */
};

/* Matrix operation a renderable applies between glMultMatrixd(link) and its draw call
 * (src/renderable.cpp:95 glTranslatef for cylinders, :128 / :427 glScalef for the second
 * box and for meshes). */
enum { RTUF_OP_NONE = 0, RTUF_OP_SCALE = 1, RTUF_OP_TRANSLATE = 2 };

/* rtuf_params.flags */
enum {
  /* (bit 0 was RTUF_FLAG_BACKGROUND_QUAD up to ABI 2.  The reference always draws the background quad at 0.99*far,
   * src/urdf_filter.cpp:591-596, and so does this library: there is nothing to switch.) */
  RTUF_FLAG_TWO_KERNEL      = 1u << 1,  /* rasteriser writes the z-surface to HBM and a separate compare kernel consumes it
                                           (default: compare fused into the tile kernel, the z-surface never leaves LDS)        */
  RTUF_FLAG_STRICT_GRID     = 1u << 2,  /* ABI 6: every set-up launch takes the worst-case grid (every chunk visible in every
                                           stream) instead of one sized from the previous batch's work lists, so a batch is never
                                           run again because its work list outgrew the estimate (RTUF_STATUS_GRID_SHORT cannot
                                           happen).  Costs empty workgroups: for consumers that read device planes before the
                                           host has retired the batch (rtuf_batch_status_device) and want one reason less for a
                                           provisional batch */
  RTUF_FLAG_DEFAULT = 0
  /* Any other bit makes rtuf_create / rtuf_set_params fail with RTUF_ERR_INVALID.  (The kernels' timing experiments
   * live only in a separate library built with -DRTUF_ABLATE for scripts/ablate_*.sh; the product has no such code.) */
};

/* Replaces the constructor's rosparam parsing (src/urdf_filter.cpp:43-118) and the
 * hard-coded clip planes (:53-54). */
typedef struct {
  float near_plane;                 /* 0.1  */
  float far_plane;                  /* 8.0  */
  float depth_distance_threshold;   /* rosparam depth_distance_threshold -> shader uniform max_diff (:630) */
  float filter_replace_value;       /* rosparam filter_replace_value     -> shader uniform replace_value (:631) */
  uint32_t flags;                   /* RTUF_FLAG_* */
  uint32_t bin_capacity;            /* triangles per (stream, screen tile) bin to start with; 0 = automatic (1024); grown from what
                                       the first batches ask for */
  uint32_t max_inflight_streams;    /* streams rasterised per internal launch group (= streams a raster lane's bins are sized for);
                                       0 = automatic: max_streams divided by the raster lanes (256 streams, three lanes: three
                                       groups of 86, one per lane), the whole batch up to 1024 with one lane; fewer if the bins
                                       would exceed a third of the free device memory or memory_limit_mb.  Smaller groups trade
                                       frames/s for memory: 256 VGA streams of a 250 k-triangle robot run at 514-525 k frames/s
                                       in 8.9 GB with three groups of 86, at 480 k in 4.5 GB with six groups of 43 (490 k in
                                       4.45 GB with two lanes and four groups of 64) */
  uint32_t pipelines;               /* 0 / 1: one raster pipeline.  2..4: that many complete pipelines (HIP streams, bins,
                                       staging, geometry copy) inside the context; batches alternate between them, so the
                                       small and low-occupancy kernels of one batch (pose stage, cull, clip, kernel tails)
                                       run underneath another batch's set-up / tile kernels (+10 % frames/s with 2 on the
                                       256-stream VGA workload).  Setters apply to all pipelines; up to 2 x pipelines batches
                                       may be in flight; rtuf_filter() and the debug read-backs use the first / the last-used
                                       pipeline.  Fixed at rtuf_create. */
  /* ABI 5 */
  uint32_t raster_lanes;            /* 0 = automatic (3; at most 3).  A raster lane is a HIP stream plus a set of tile bins sized for
                                       ONE launch group.  With several, a batch of >= 32 streams is split into launch groups (a
                                       multiple of the lanes) that alternate between the lanes, which run free of each other: every
                                       kernel's ramp, tail and launch gap is filled by the other lanes' kernels.  Smaller batches
                                       take one lane each, in turn.  Three lanes and the pose stage's stream are one HIP stream per
                                       hardware queue of the runtime's default four (GPU_MAX_HW_QUEUES).  1 = one lane, every kernel
                                       alone on the GPU (what per-kernel timings and rooflines should be measured with).  Fixed at
                                       rtuf_create. */
  uint32_t memory_limit_mb;         /* upper bound of the rasteriser's working set (tile bins of all lanes), MiB; 0 = a third of
                                       the free device memory at rtuf_finalize_models.  When the bins a scene needs would exceed it
                                       the launch groups shrink (more, smaller launches) instead of the call failing; when even
                                       one stream's bins are larger the bins are grown all the same (up to what the device has)
                                       and rtuf_stats.over_memory_limit says so. */
  uint32_t silhouette_dilation_px;  /* 0 .. 16 (was reserved[0], same offset; 0 = off, the reference's behaviour).  New, beyond the
                                       reference, like the batch and lane entries: widens the rendered robot by r pixels to cover
                                       mixed depth pixels at the sensor's edges, camera_offset calibration error and TF latency.
                                       For r > 0 every pixel p of a stream is shaded with z'(p) instead of its own window z: the
                                       smallest drawn z in the (2r+1) x (2r+1) square around p, clipped to that stream's image
                                       (never padded, never reaching into another stream), and "nothing drawn" when the square
                                       holds nothing drawn.  The outputs are then exactly the shader's for z': filtered where
                                       sensor > to_linear_depth(z') - depth_distance_threshold, masked 0 / mask 0 (the GL clear
                                       colour) where nothing is drawn.  z' is always one of the square's own values, so the depth
                                       test still decides: a foreground object in front of the widened silhouette is kept.  The
                                       background quad is drawn, so away from the robot nothing changes; a pixel the background does
                                       not cover (a non-standard projection) with a drawn pixel within r becomes drawn.  Batches
                                       run the z-surface route (tile kernel writes the window z, a dilate-and-compare kernel makes
                                       every output form, mask bits included) whatever RTUF_FLAG_TWO_KERNEL says, one batch in
                                       flight at a time.  Larger values fail with RTUF_ERR_INVALID. */
  uint32_t reserved[1];
} rtuf_params;

void rtuf_default_params(rtuf_params *p);
int rtuf_abi_version(void);

/* ctor + initGL() + initFrameBufferObject() (src/urdf_filter.cpp:43-118, :386-456):
 * binds a GPU, allocates the per-stream frame resources for `max_streams` concurrent
 * width x height depth streams.  No GL / X11 context exists anywhere. */
int rtuf_create(rtuf_context **out, int device_id, int width, int height, int max_streams,
                const rtuf_params *params);
void rtuf_destroy(rtuf_context *ctx);
const char *rtuf_last_error(const rtuf_context *ctx);

/* Uniforms can change between frames like the public data members of the reference
 * (include/realtime_urdf_filter/urdf_filter.h:112-135).  far_plane is the exception: the background
 * quad is part of the finalized geometry, so changing it after rtuf_finalize_models returns
 * RTUF_ERR_STATE. */
int rtuf_set_params(rtuf_context *ctx, const rtuf_params *params);

/* ---- geometry: loaded once into device buffers ------------------------------------
 * loadModels() -> URDFRenderer ctor -> process_link -> Renderable* ctor
 * (src/urdf_filter.cpp:127-197, src/urdf_renderer.cpp:44-169, src/renderable.cpp:100-170,
 * :306-415).  A model is one `models[i]` entry (one URDFRenderer); a link is one
 * Renderable (one glPushMatrix/glPopMatrix bracket, posed per frame by its
 * link_to_fixed * link_offset matrix); a draw is one GL draw call inside that bracket.
 * Geometry is already tessellated into indexed triangles, in draw order. */
int rtuf_add_model(rtuf_context *ctx);                       /* returns model id >= 0 */
int rtuf_add_link(rtuf_context *ctx, int model);             /* returns link id >= 0 (index within the model) */
int rtuf_add_draw(rtuf_context *ctx, int model, int link, int pre_op, const float op_xyz[3],
                  const float *vertices_xyz, int n_vertices,
                  const uint32_t *triangles, int n_triangles);
/* Uploads everything added so far (VBO/IBO creation, src/renderable.cpp:167-169, :343-349). */
int rtuf_finalize_models(rtuf_context *ctx);
int rtuf_num_links(const rtuf_context *ctx, int model);
int64_t rtuf_num_triangles(const rtuf_context *ctx);
/* Vertices resident on the device after rtuf_finalize_models: per set-up chunk (<= 256 triangles) every distinct position
 * once (bit-identical positions of one draw are merged: STL facets bring three vertices of their own each, which the
 * reference uploads as they are, src/renderable.cpp:339-350; the image cannot tell), plus the background quad's four. */
int64_t rtuf_num_vertices(const rtuf_context *ctx);

/* Which models a stream renders (default: all).  Lets independent robots share a context
 * (BASELINE config 5); the reference renders every loaded model for its single stream. */
int rtuf_set_stream_models(rtuf_context *ctx, int stream, const int *model_ids, int n_models);

/* ---- per-frame pose inputs -------------------------------------------------------- */
/* Camera of one stream: projection = getProjectionMatrix() result (src/urdf_filter.cpp:459-501);
 * camera_offset_inv = inverse(camera_offset).getOpenGLMatrix() (:602-604);
 * camera_tf = camera_transform.getOpenGLMatrix() after the tx/ty origin shift (:607-614).
 * Composed on the device in float32 in OpenGL matrix-stack order. */
int rtuf_set_camera(rtuf_context *ctx, int stream, const double projection[16],
                    const double camera_offset_inv[16], const double camera_tf[16]);
/* K (fx,fy,cx,cy,Tx,Ty) -> projection[16] and camera_tx/ty, exactly getProjectionMatrix. */
void rtuf_projection_from_intrinsics(double fx, double fy, double cx, double cy, double Tx, double Ty,
                                     int width, int height, double near_plane, double far_plane,
                                     double projection_out[16], double *camera_tx, double *camera_ty);
/* Link poses of one model for one stream: n_links matrices
 * (link_to_fixed * link_offset).getOpenGLMatrix(), i.e. what Renderable::applyTransform
 * passes to glMultMatrixd (src/renderable.cpp:59-68) after URDFRenderer::update_link_transforms
 * (src/urdf_renderer.cpp:173-190). */
int rtuf_set_link_poses(rtuf_context *ctx, int stream, int model, const double *link_tf, int n_links);

/* Batched forms of the two setters above (one FFI crossing per frame for N streams):
 * matrices are [n_streams][16] resp. [n_streams][n_links][16], for streams
 * first_stream .. first_stream + n_streams - 1.  Any of the three camera arrays may be NULL
 * (that matrix keeps its previous value for all n streams). */
int rtuf_set_cameras(rtuf_context *ctx, int first_stream, int n_streams, const double *projection,
                     const double *camera_offset_inv, const double *camera_tf);
int rtuf_set_link_poses_batch(rtuf_context *ctx, int first_stream, int n_streams, int model,
                              const double *link_tf, int n_links);
/* camera_tx_ / camera_ty_ of getProjectionMatrix (src/urdf_filter.cpp:481-482) for streams whose camera transform
 * is derived on the device (rtuf_set_joint_positions with camera_frame >= 0): the forward-kinematics kernel moves
 * the camera origin by tx along the transform's x axis and ty along its y axis, src/urdf_filter.cpp:607-611.
 * (A camera_tf handed to rtuf_set_camera(s) has the shift applied by the caller already and is not touched.)
 * NULL = 0 for all n streams. */
int rtuf_set_camera_shift(rtuf_context *ctx, int first_stream, int n_streams, const double *camera_tx,
                          const double *camera_ty);

/* ---- on-device forward kinematics --------------------------------------------------
 * Replaces the per-renderable TF lookups of URDFRenderer::update_link_transforms
 * (src/urdf_renderer.cpp:173-190) for robots whose link poses follow from joint positions: the
 * kinematic tree of a model is uploaded once, per frame only the joint positions cross the bus and
 * a kernel computes every  fixed<-link  transform and the matrices of rtuf_set_link_poses on the GPU
 * (double precision, same multiplication order as the host-side forward kinematics).
 *   n_frames frames, parent[i] < i or -1 for the root; joint_type 0 fixed, 1 revolute/continuous,
 *   2 prismatic; joint_origin[i] = parent<-child transform at q = 0 (column-major); joint_axis[i] in
 *   the child frame; link_frame[l] = frame the l-th link (renderable) of the model is attached to;
 *   link_offset[l] = the URDF <origin> of its visual/collision (Renderable::link_offset). */
enum { RTUF_JOINT_FIXED = 0, RTUF_JOINT_REVOLUTE = 1, RTUF_JOINT_PRISMATIC = 2 };
int rtuf_set_kinematics(rtuf_context *ctx, int model, int n_frames, const int32_t *parent,
                        const int32_t *joint_type, const double *joint_origin, const double *joint_axis,
                        const int32_t *link_frame, const double *link_offset, int n_links);
/* Joint positions q[n_streams][n_frames] (entries of fixed joints are ignored) and, optionally, the
 * pose of the root frame in the fixed frame root_tf[n_streams][16] (NULL = identity).  With
 * camera_frame >= 0 the camera transform of each stream becomes inverse(fixed<-camera_frame)
 * (a camera mounted on the robot, shifted by rtuf_set_camera_shift); with -1 it is what rtuf_set_camera(s) set
 * (also again after an earlier call with camera_frame >= 0).  Overrides
 * rtuf_set_link_poses for this model on these streams until rtuf_set_link_poses is called again. */
int rtuf_set_joint_positions(rtuf_context *ctx, int first_stream, int n_streams, int model, const double *q,
                             const double *root_tf, int camera_frame);
/* Debug / test access: the link matrices ([n_streams][total links][16]) and camera transforms
 * ([n_streams][16]) the last batch was rendered with. */
int rtuf_debug_read_poses(rtuf_context *ctx, int n_streams, double *link_tf_out, double *cam_tf_out);

/* ---- the hot path ------------------------------------------------------------------ */
/* filter() for n streams at once (stream ids 0..n-1), host buffers:
 * depth_in[s]: width*height float32 metres, row 0 first (src/urdf_filter.cpp:233-234);
 * masked_out[s]: width*height float32 (getMaskedDepth()); mask_out may be NULL, or
 * mask_out[s] NULL (need_mask_ == false, :226-230), else width*height bytes 0/255. */
int rtuf_filter_batch(rtuf_context *ctx, int n_streams, const float *const *depth_in,
                      float *const *masked_out, uint8_t *const *mask_out);
/* Same with device-resident planes: depth/masked are [n][H][W] float32, mask [n][H][W] u8 or
 * NULL.  Asynchronous on the context's stream.  Up to two batches may be in flight: a call made
 * while two are pending first retires the oldest (as rtuf_sync does for all of them), so a caller
 * that keeps enqueueing never leaves the GPU idle during the host round trip.  The buffers of a
 * batch must stay valid and unmodified until it is retired (a bin regrowth runs it again);
 * the per-frame pose setters -- rtuf_set_joint_positions, rtuf_set_camera(s), rtuf_set_camera_shift,
 * rtuf_set_link_poses[_batch] -- may be called at any time: their staging is a ring of sets, one per batch in
 * flight plus one being written, so the next frame's poses are staged while the GPU filters this one (only a call
 * that switches a stream between forward kinematics and explicit matrices waits).  Every other setter (parameters,
 * model selection, kinematic trees) waits for the batches in flight.  rtuf_sync() retires everything in flight.
 * ORDER OF BATCHES IN FLIGHT: none.  With more than one raster lane (the default) consecutive batches run on different
 * HIP streams -- a batch of one launch group takes the lanes in turn -- and nothing orders the kernels of one batch behind
 * those of the batch before it.  Two batches in flight must therefore not share an output plane, and a batch must not read
 * as its sensor plane what the batch before it writes: retire the first (rtuf_wait_oldest / rtuf_sync) or run the context with
 * rtuf_params.raster_lanes = 1, where batches execute in the order they were enqueued. */
int rtuf_filter_batch_device(rtuf_context *ctx, int n_streams, const float *d_depth,
                             float *d_masked, uint8_t *d_mask);
/* 16UC1 variants: depth in / out as uint16 millimetres with the reference's conversions fused into the
 * kernels (filter_callback, src/urdf_filter.cpp:280-289: convertTo(CV_32F, 0.001); :308-312:
 * convertTo(CV_16U, 1000.0), i.e. filtered pixels become filter_replace_value * 1000).  Halves the
 * HBM and PCIe bytes per pixel (5 instead of 9). */
int rtuf_filter_batch_u16(rtuf_context *ctx, int n_streams, const uint16_t *const *depth_mm_in,
                          uint16_t *const *masked_mm_out, uint8_t *const *mask_out);
/* Asynchronous forms of the two host-plane calls: the planes go up on one copy stream and come back on
 * another, so with two batches in flight the PCIe transfers of one overlap the kernels of the other
 * (the reference uploads, renders and reads back serially: src/urdf_filter.cpp:332-353, :729-735).
 * All planes of a batch must stay valid until it is retired -- by rtuf_wait_oldest, rtuf_sync, or
 * the second-next asynchronous call -- and should be pinned memory (rtuf_host_alloc); with pageable
 * memory the calls are correct but block for the transfers.  Planes that follow each other in memory
 * are moved as one transfer. */
int rtuf_filter_batch_async(rtuf_context *ctx, int n_streams, const float *const *depth_in,
                            float *const *masked_out, uint8_t *const *mask_out);
int rtuf_filter_batch_u16_async(rtuf_context *ctx, int n_streams, const uint16_t *const *depth_mm_in,
                                uint16_t *const *masked_mm_out, uint8_t *const *mask_out);
/* ---- mask-only output, one bit per pixel -----------------------------------------------------------------
 * The reference publishes the mask on its own topic (src/urdf_filter.cpp:321-329) and the masked depth is a pure
 * function of sensor plane and mask: masked = mask ? filter_replace_value : sensor (tests check this bit for bit on
 * every full-plane result).  These calls return ONLY the mask, packed: pixel (x, y) of a stream is bit x % 32 of
 * 32-bit word y * ceil(width / 32) + x / 32 (rtuf_mask_bits_words() words per stream).  Device-to-host traffic per
 * VGA frame drops from 1.54 MB to 38 KB, which turns the PCIe-bound host-plane path from download-bound into
 * upload-bound; rtuf_expand_mask_bits() rebuilds masked depth and/or the byte mask of a frame on the host where and
 * when a consumer needs them.  Not with RTUF_FLAG_TWO_KERNEL (silhouette dilation is fine); width must be a multiple of 4.  Exactness: the identity above holds
 * wherever the background quad covers the image -- every getProjectionMatrix() camera.  For a projection where it
 * does not (pixels the reference leaves at the GL clear colour 0), retiring the batch fails with RTUF_ERR_STATE
 * instead of returning bits that would expand to something else. */
size_t rtuf_mask_bits_words(int width, int height);
int rtuf_filter_batch_bits_async(rtuf_context *ctx, int n_streams, const float *const *depth_in, uint32_t *const *bits_out);
int rtuf_filter_batch_bits_u16_async(rtuf_context *ctx, int n_streams, const uint16_t *const *depth_mm_in,
                                     uint32_t *const *bits_out);
/* device-resident planes: depth [n][H][W], bits [n][rtuf_mask_bits_words()] */
int rtuf_filter_batch_device_bits(rtuf_context *ctx, int n_streams, const float *d_depth, uint32_t *d_bits);
int rtuf_filter_batch_device_bits_u16(rtuf_context *ctx, int n_streams, const uint16_t *d_depth_mm, uint32_t *d_bits);
/* Host helper (no GPU, no context): one frame's masked depth (float32, or uint16 millimetres with the reference's
 * convertTo arithmetic when is_u16) and/or 0/255 byte mask from its sensor plane and mask bits.  Either output may
 * be NULL. */
int rtuf_expand_mask_bits(const void *depth_in, int is_u16, const uint32_t *bits, int width, int height,
                          float replace_value, void *masked_out, uint8_t *mask_out);

/* Waits for the oldest batch in flight (device or host planes); its outputs are complete afterwards.
 * RTUF_OK when nothing is pending. */
int rtuf_wait_oldest(rtuf_context *ctx);
/* Pinned host memory for the asynchronous calls.  rtuf_host_free waits for the batches in flight. */
int rtuf_host_alloc(rtuf_context *ctx, size_t bytes, void **out);
int rtuf_host_free(rtuf_context *ctx, void *ptr);
int rtuf_filter_batch_device_u16(rtuf_context *ctx, int n_streams, const uint16_t *d_depth_mm,
                                 uint16_t *d_masked_mm, uint8_t *d_mask);
/* Exact single-stream shape of RealtimeURDFFilter::filter(buffer, glTf, w, h)
 * (include/realtime_urdf_filter/urdf_filter.h:70-72): stream 0, projection given per call,
 * results kept in library-owned host buffers like masked_depth_/mask_. */
int rtuf_filter(rtuf_context *ctx, const unsigned char *buffer, const double *projection,
                int width, int height);
const float *rtuf_get_masked_depth(const rtuf_context *ctx);      /* getMaskedDepth() */
const uint8_t *rtuf_get_mask(const rtuf_context *ctx);            /* mask_ */

int rtuf_sync(rtuf_context *ctx);
/* The HIP stream the raster stage of this context is enqueued on -- defined only for a context of ONE raster lane and ONE
 * pipeline (rtuf_params.raster_lanes = 1, pipelines <= 1).  Every other context spreads a batch over several internal
 * streams and returns NULL here: do NOT pass that NULL to hipStreamWaitEvent / hipEventRecord (NULL is the legacy default
 * stream there: nothing fails and the ordering is simply wrong).  Callers that order their own device work behind the
 * batches use rtuf_order_stream_after_batches() instead, which is right for every configuration. */
void *rtuf_stream(rtuf_context *ctx);
/* Makes `hip_stream` (a hipStream_t of the context's device; NULL = the legacy default stream) wait, on the device, for
 * every batch enqueued on this context so far: all raster lanes, all pipelines, and for host-plane batches their
 * downloads.  Does not block the host and does not retire anything (the batches' buffers stay owned by the library until
 * rtuf_wait_oldest / rtuf_sync).  ABI 5.
 *
 * WHAT THIS DOES NOT GUARANTEE: that the planes are final.  The rasteriser's working buffers (tile bins, clip list, many-tile
 * list, the set-up grid) are sized from what earlier batches needed; whether a batch outgrew one of them is known only once
 * its kernels have run, and the HOST acts on it when it retires the batch (rtuf_wait_oldest / rtuf_sync / the second-next
 * filter call): it enlarges the buffer and runs the batch again into the same planes.  Until then the planes of such a batch
 * hold pixels of a rasterisation that dropped triangles.  The reference's filter() returns with final pixels
 * (src/urdf_filter.cpp:237, :729-735); so do all calls here that retire through the host.  A consumer that reads device
 * planes behind this call, before the host has retired the batch, must check the batch's STATUS WORD on the device: */
int rtuf_order_stream_after_batches(rtuf_context *ctx, void *hip_stream);
/* ABI 6.  Device address of the status word (one uint32) of the batch the most recent rtuf_filter_batch* call enqueued
 * (with pipelines: of the pipeline that took it).  The planes of that batch are final IF AND ONLY IF the word reads 0
 * after the batch's kernels -- i.e. on a stream ordered behind them with rtuf_order_stream_after_batches.  Otherwise:
 *   bits 0..15   launch groups of the batch that have not finished yet (non-zero only for a reader that is NOT ordered behind
 *                the batch, or while the library runs the batch again)
 *   RTUF_STATUS_*_OVERFLOW / _GRID_SHORT   a working buffer was too small: the planes are provisional, and the library will
 *                run the batch again when the host retires it; the word reads 0 once that run has finished
 *   RTUF_STATUS_UNCOVERED   mask-bits output only: the bits do not expand to the reference's planes (retiring the batch fails)
 * The address belongs to one of the context's two batch slots: it is reused by the second-next batch, whose first kernel
 * overwrites the word -- read it in the same stream-ordered work that reads the planes.  rtuf_stats.batch_status is the
 * host's mirror for the batch retired last (what its first run left in the word). */
enum {
  RTUF_STATUS_PENDING_MASK  = 0xffffu,
  RTUF_STATUS_BIN_OVERFLOW  = 1u << 16,   /* a (stream, tile) bin held more records or fragments than its capacity      */
  RTUF_STATUS_CLIP_OVERFLOW = 1u << 17,   /* more triangles crossed a frustum plane than the clip list holds             */
  RTUF_STATUS_LIST_OVERFLOW = 1u << 18,   /* more many-tile records than their list holds                               */
  RTUF_STATUS_GRID_SHORT    = 1u << 19,   /* a launch group's work list outgrew the set-up grid sized from the last batch */
  RTUF_STATUS_UNCOVERED     = 1u << 20    /* rtuf_filter_batch*_bits*: a pixel no fragment reached                       */
};
int rtuf_batch_status_device(rtuf_context *ctx, const uint32_t **d_status);

/* LINK LABELS.  New, beyond the reference: which robot link every pixel shows, as a uint16_t plane [n][H][W] (row 0 first)
 * beside the masked depth.  A pixel's label is the label of the link whose fragment won its depth test -- GL_LESS on the
 * 24-bit depth, ties going to the earlier draw: exactly the winner the planes are shaded with.  Label 0: the background
 * quad won, or nothing was drawn.  The label does not depend on the sensor plane or the threshold; combine it with the mask
 * (mask 255 with label 0 = filtered by the background quad, i.e. the sensor reads beyond the far plane).
 * Default labels: link l of model m is 1 + link_base(m) + l, where link_base(m) counts the links of the models added before m
 * (the order rtuf_add_model / rtuf_add_link create them in).  A context with more than 65535 links fails the label calls with
 * RTUF_ERR_CAPACITY unless rtuf_set_link_labels has given labels to the models whose defaults would not fit.
 * rtuf_set_link_labels overrides the labels of one model's links (n_links = rtuf_num_links(model)): any value, 0 ("do not
 * label this link") and values shared by several links (grouping) included.  It waits for the batches in flight.
 * The label calls take the arguments of their counterparts plus the label planes (device: [n][H][W], 8-byte aligned; host:
 * one width*height plane per stream, never NULL) and write masked / mask bit for bit as the counterparts do, mask may be NULL.
 * Both RTUF_FLAG_TWO_KERNEL settings, any number of raster lanes and pipelines; re-runs after a bin regrowth rewrite the
 * labels with the planes, and the status word (rtuf_batch_status_device) covers the label plane with the same meaning.
 * Not supported yet: silhouette_dilation_px > 0 (RTUF_ERR_INVALID).  There are no label forms of the mask-bits calls or of
 * the asynchronous host-plane calls; the host-plane label calls are synchronous.  The draw-order -> label table they use
 * (2 bytes per triangle) is allocated by the first label call or rtuf_set_link_labels. */
int rtuf_set_link_labels(rtuf_context *ctx, int model, const uint16_t *labels, int n_links);
int rtuf_filter_batch_device_labels(rtuf_context *ctx, int n_streams, const float *d_depth, float *d_masked, uint8_t *d_mask,
                                    uint16_t *d_labels);
int rtuf_filter_batch_device_u16_labels(rtuf_context *ctx, int n_streams, const uint16_t *d_depth_mm, uint16_t *d_masked_mm,
                                        uint8_t *d_mask, uint16_t *d_labels);
int rtuf_filter_batch_labels(rtuf_context *ctx, int n_streams, const float *const *depth_in, float *const *masked_out,
                             uint8_t *const *mask_out, uint16_t *const *labels_out);
int rtuf_filter_batch_u16_labels(rtuf_context *ctx, int n_streams, const uint16_t *const *depth_mm_in,
                                 uint16_t *const *masked_mm_out, uint8_t *const *mask_out, uint16_t *const *labels_out);

/* PER-LINK DEPTH THRESHOLDS.  New, beyond the reference: a depth_distance_threshold (the shader's max_diff) of its own for
 * every link of a model -- a wide margin for a gripper holding an object, a tight one for a wall, none at all for a link a
 * tracker must still see.  A drawn pixel is compared with the threshold of the link whose fragment won its depth test (GL_LESS
 * on the 24-bit depth, ties going to the earlier draw: the winner the link labels report): sensor > to_linear_depth(z) - t,
 * the shader's compare with the same float operations and t in place of max_diff.  Pixels the background quad won keep
 * rtuf_params.depth_distance_threshold; undrawn pixels stay the GL clear colour.
 * Any float is legal.  A larger t filters more: -inf and NaN never filter the link (the compare is false), +inf filters every
 * pixel where it is drawn and the sensor is not NaN; 0 and negative values are ordinary margins.
 * rtuf_set_link_thresholds sets the thresholds of one model's links (n_links = rtuf_num_links(model)).
 * rtuf_clear_link_thresholds makes the model's links follow rtuf_params again.  Links without a value -- models never given
 * thresholds, or cleared -- use the global threshold of every batch, so a later rtuf_set_params that changes it applies to
 * them and not to links set explicitly.  Both calls wait for the batches in flight; a bad model id, a wrong n_links or a NULL
 * array fail with RTUF_ERR_INVALID and change nothing.
 * The thresholds apply to every fused entry point: rtuf_filter, the f32 and 16UC1 device and host-plane calls (synchronous
 * and asynchronous), the mask-bits calls (the replace value stays global, so rtuf_expand_mask_bits stays exact) and the link
 * label calls.  Any number of raster lanes and pipelines; re-runs after a bin regrowth keep the thresholds, and the status
 * word (rtuf_batch_status_device) keeps its meaning.
 * Not supported yet: while any model of the context has thresholds, a batch with RTUF_FLAG_TWO_KERNEL or
 * silhouette_dilation_px > 0 fails with RTUF_ERR_INVALID before anything is enqueued (the z-surface does not carry the winning
 * link).  While no model has thresholds -- after the last rtuf_clear_link_thresholds too -- nothing differs from a context that
 * never used them.  The draw-order -> threshold table (4 bytes per triangle) is allocated by the first rtuf_set_link_thresholds. */
int rtuf_set_link_thresholds(rtuf_context *ctx, int model, const float *depth_distance_threshold, int n_links);
int rtuf_clear_link_thresholds(rtuf_context *ctx, int model);

/* VIRTUAL DEPTH.  New, beyond the reference: the robot's own depth image -- to_linear_depth(gl_FragCoord.z) of
 * include/shaders/urdf_filter.frag:22, the metric depth at which the model puts the robot in every pixel -- as a plane
 * [n][H][W] (row 0 first), with no sensor plane read and nothing compared.  Streams 0 .. n-1 are posed by the same setters as
 * a filter batch.  A pixel's winner is the filter's: GL_LESS on the 24-bit depth, ties going to the earlier draw.
 * Where a link's fragment won: virtual = num / (z - off), z the float window z the compare uses, num / off the shader's
 * z_near*z_far/(z_near-z_far) and z_far/(z_far-z_near) in float -- the operations of the compare threshold without its final
 * subtraction, bit for bit, so sensor > virtual - t reproduces the mask of a filter batch with threshold t.
 * Where the background quad won, or nothing was drawn: empty_value as given; any float is legal, NaN and +-inf included.
 * The 16UC1 forms (width a multiple of 4) write uint16 millimetres: every value, empty_value included, goes through the
 * conversion the masked 16UC1 output applies (round half to even, saturating, NaN and out of int range -> 0).
 * Labels: d_labels may be NULL; labels_out is NULL or one plane per stream.  When given it is exactly the plane the label
 * calls write (LINK LABELS: default labels, rtuf_set_link_labels, the > 65535 links rule, the table allocated on first use;
 * device: [n][H][W], 8-byte aligned).  sensor - virtual where labels > 0 is the calibration residual of the links.
 * depth_distance_threshold, filter_replace_value, per-link thresholds and RTUF_FLAG_TWO_KERNEL do not enter: a render batch
 * is always one tile kernel, never touches the z-surface (rtuf_debug_read_zsurface keeps showing the last filter batch), and
 * is accepted on a context with per-link thresholds or the two-kernel flag set.
 * Otherwise a render batch is a batch like any other: raster lanes, pipelines, launch groups, as many in flight as the
 * context's filter batches, partial batches, re-runs after a bin regrowth into the same planes with the same empty_value,
 * the status word (rtuf_batch_status_device) and rtuf_stats with their meaning (timings: ms_raster),
 * rtuf_order_stream_after_batches; no order between batches in flight, render or filter.  The host-plane forms are
 * synchronous.  Not supported yet: silhouette_dilation_px > 0 (RTUF_ERR_INVALID).  A NULL plane, n out of range or an
 * un-finalized context fail as the filter calls do; a refused call enqueues nothing. */
int rtuf_render_batch_device(rtuf_context *ctx, int n_streams, float *d_virtual, uint16_t *d_labels, float empty_value);
int rtuf_render_batch_device_u16(rtuf_context *ctx, int n_streams, uint16_t *d_virtual_mm, uint16_t *d_labels, float empty_value);
int rtuf_render_batch(rtuf_context *ctx, int n_streams, float *const *virtual_out, uint16_t *const *labels_out, float empty_value);
int rtuf_render_batch_u16(rtuf_context *ctx, int n_streams, uint16_t *const *virtual_mm_out, uint16_t *const *labels_out,
                          float empty_value);

/* LINK RESIDUAL TABLES.  New, beyond the reference: per stream and link label, how the sensor plane compares with the model
 * -- how many pixels the link covers, how many the sensor confirms, how many show something in front of the link or see
 * through it, how many hold no reading, and the summed residual sensor - virtual of the confirmed ones -- as a table
 * [n_streams][n_labels] of 64-byte rows, with no plane written at all.  Streams 0 .. n-1 are posed by the same setters as a
 * filter batch.  Row l of stream s collects the pixels of s whose label is l, the label rtuf_filter_batch*_labels would write
 * (LINK LABELS: same winner, default labels or rtuf_set_link_labels, the > 65535 links rule, the table allocated on first
 * use); row 0 covers the background quad, pixels nothing was drawn to, and links labelled 0.  Every call overwrites its
 * table (rows no pixel reaches are zero); it never accumulates into what was there.  All sums are integers: the table does
 * not depend on the order of execution.
 * Per pixel, s = the sensor value (the float as given; 16UC1: uint16 * 0.001f, as every 16UC1 call reads it):
 *   no fragment reached the pixel:  pixels++, and invalid++ if !(s > 0); nothing else.
 *   drawn pixel (the background quad included), z the float window z the filter uses, t the threshold the filter would
 *   use (the winner's link threshold where rtuf_set_link_thresholds gave one, else depth_distance_threshold),
 *   v = num / (z - off) (VIRTUAL DEPTH), lo = v - t and hi = v + t (one float operation each):
 *     valid = s > 0;  filtered = s > lo  (the filter's mask, for an invalid s as well);
 *     in_front = valid && !filtered;  behind = valid && filtered && s > hi;  agree = valid && filtered && !(s > hi);
 *     agree pixels add q = round_half_even((s - v) * 2^20) (float subtraction and product; saturating to int32, NaN -> 0)
 *     to sum_residual and |q| to sum_abs_residual: sum_residual / agree * 2^-20 is the mean signed residual in metres.
 *   For rows without undrawn pixels invalid + in_front + behind + agree == pixels.
 * With t NaN or -inf every valid pixel of that link counts as in_front; with t = +inf every valid pixel counts as agree, and
 * q saturates where the residual is 2048 m or more.
 * Refusals, each enqueuing nothing and leaving the table untouched: a link of the context whose label is >= n_labels, or
 * n_labels < 1 (RTUF_ERR_INVALID; the label table is checked on the host); silhouette_dilation_px > 0 (RTUF_ERR_INVALID); a
 * NULL plane or table, n out of range, an un-finalized context, a 16UC1 call with a width that is not a multiple of 4, as
 * the filter calls.
 * RTUF_FLAG_TWO_KERNEL and filter_replace_value do not enter: a residual batch is always one tile kernel, never touches the
 * z-surface, and is accepted on a context with per-link thresholds (honoured) and with the two-kernel flag.  Otherwise it is
 * a batch like any other: raster lanes, pipelines, launch groups, partial batches, batches in flight (each with a table of
 * its own), graph replay of small batches, re-runs after a bin regrowth (the table is zeroed again: as if the batch had run
 * once), the status word and rtuf_stats with their meaning (timings: ms_raster), rtuf_order_stream_after_batches.  The
 * device forms only enqueue (d_table: [n][n_labels], 8-byte aligned); the host-plane forms are synchronous: planes up,
 * table down. */
typedef struct {
  uint64_t pixels;           /* pixels of the stream whose label is this row's                                      */
  uint64_t invalid;          /* ... whose sensor value is not > 0 (NaN, 0, negative)                                */
  uint64_t filtered;         /* ... the filter would mask: exactly the pixels with mask 255                         */
  uint64_t in_front;         /* valid, not filtered: the sensor sees something nearer than the link by more than t  */
  uint64_t behind;           /* valid, filtered, sensor > virtual + t: the sensor sees through the link             */
  uint64_t agree;            /* valid, filtered, not behind: the sensor confirms the link                           */
  int64_t sum_residual;      /* over the agree pixels: sum of q, q = (sensor - virtual) in units of 2^-20 m         */
  uint64_t sum_abs_residual; /* over the agree pixels: sum of |q|                                                   */
} rtuf_link_residuals;       /* 64 bytes */

int rtuf_link_residuals_batch_device(rtuf_context *ctx, int n_streams, const float *d_depth, rtuf_link_residuals *d_table, int n_labels);
int rtuf_link_residuals_batch_device_u16(rtuf_context *ctx, int n_streams, const uint16_t *d_depth_mm, rtuf_link_residuals *d_table,
                                         int n_labels);
int rtuf_link_residuals_batch(rtuf_context *ctx, int n_streams, const float *const *depth_in, rtuf_link_residuals *table_out, int n_labels);
int rtuf_link_residuals_batch_u16(rtuf_context *ctx, int n_streams, const uint16_t *const *depth_mm_in, rtuf_link_residuals *table_out,
                                  int n_labels);

/* FILTERED POINT CLOUDS.  New, beyond the reference: the pixels the filter keeps, as XYZ points in the camera's optical
 * frame -- what the filter's consumers (octomap, MoveIt, trackers) take -- either organized (one point per pixel, NaN where
 * there is none) or compacted (the kept points of every stream, densely, in row-major order, with their count).
 * Intrinsics.  rtuf_set_cloud_intrinsics stores, for streams first_stream .. first_stream + n_streams - 1, four floats from
 * fx_fy_cx_cy [n][4]: kx = (float)(1.0 / fx), ky = (float)(1.0 / fy), cx = (float)cx, cy = (float)cy.  An fx or fy that is
 * not finite or not > 0 (and a NULL array or a stream range outside the context) fails with RTUF_ERR_INVALID and changes
 * nothing.  The call waits for the batches in flight, as the other non-pose setters do, and applies to all pipelines.  A
 * cloud call on a stream that never got intrinsics fails with RTUF_ERR_STATE and enqueues nothing.
 * A point.  s = the sensor value (the float as given; 16UC1: uint16 * 0.001f, as every 16UC1 call reads it).  Pixel (u, v),
 * row 0 first, is KEPT iff its mask bit is 0 -- the filter batch of the same parameters would not mask it -- and
 * s > 0 && s < +inf.  Its point is
 *   x = (((float)u - cx) * s) * kx,   y = (((float)v - cy) * s) * ky,   z = s,
 * every operation a single float operation in that order (as depth_image_proc associates them; cloud_point in
 * rtuf_numerics.h).  filter_replace_value does not enter.
 * Organized form (rtuf_cloud_batch_device*): d_points is [n][H][W][3] float; a kept pixel holds its point, every other pixel
 * three quiet NaNs (0x7fc00000).
 * Its device forms need d_points 16-byte aligned and d_depth 16-byte aligned (f32) or 8-byte aligned (16UC1) -- the kernel
 * loads four sensor values and stores four floats at once -- else RTUF_ERR_INVALID; the compacted forms need no more than
 * the elements' own alignment.
 * Compacted form (rtuf_cloud_compact_batch_device*): d_points is [n][capacity][3] float, d_index [n][capacity] or NULL,
 * d_counts [n].  counts[s] is the number of kept pixels of stream s -- the full number even when it exceeds capacity.  Entry
 * j of stream s is the j-th kept pixel in row-major order (organized[s][kept] in numpy terms) and is written iff
 * j < min(counts[s], capacity); d_index, when given, holds v * W + u of the same entries.  Entries at or beyond
 * min(counts[s], capacity) are unspecified (left untouched, or stale).  1 <= capacity <= W * H, else RTUF_ERR_INVALID.
 * The compaction is a count per row, a scan and a row-major scatter: no atomics, the same output on every run.
 * Host-plane forms (rtuf_cloud_batch*, rtuf_cloud_compact_batch*): synchronous, planes up, results down.  points_out is one
 * plane ([H][W][3]) or array ([capacity][3]) per stream, index_out NULL or one array per stream, counts_out [n]; the
 * compacted forms download only min(counts, capacity) entries per stream.
 * A cloud batch is a mask-bits batch plus the cloud kernels (rtuf_filter_batch_device_bits* above): the library owns the bits buffer and the
 * row scratch of the compacted form, per batch slot, allocated on first use and counted in rtuf_stats.device_bytes.  The
 * bits route's rules hold unchanged: silhouette_dilation_px is honoured (the cloud of the dilated filter), per-link
 * thresholds are honoured (not together with dilation: RTUF_ERR_INVALID), the width must be a multiple of 4
 * (RTUF_ERR_INVALID), and a stream whose background quad does not cover its image makes retiring the batch fail with
 * RTUF_ERR_STATE (RTUF_STATUS_UNCOVERED), as the bits calls do.  RTUF_FLAG_TWO_KERNEL does not enter: the batch is accepted
 * and takes the fused bits route, as render and residual batches do.  Otherwise it is a batch like any other: raster lanes,
 * pipelines, launch groups, partial batches, batches in flight (each with outputs of its own), graph replay of small
 * batches, re-runs after a bin regrowth (counts and points are rewritten: as if the batch had run once),
 * rtuf_order_stream_after_batches and the status word, which covers the cloud too (the cloud kernels run on each launch
 * group's lane before its counters are published; timings: ms_compare).  Refusals are those of the filter calls -- a NULL
 * plane, n out of range, an un-finalized context -- and a refused call enqueues nothing. */
int rtuf_set_cloud_intrinsics(rtuf_context *ctx, int first_stream, int n_streams, const double *fx_fy_cx_cy /* [n][4] */);
int rtuf_cloud_batch_device(rtuf_context *ctx, int n_streams, const float *d_depth, float *d_points);
int rtuf_cloud_batch_device_u16(rtuf_context *ctx, int n_streams, const uint16_t *d_depth_mm, float *d_points);
int rtuf_cloud_compact_batch_device(rtuf_context *ctx, int n_streams, const float *d_depth, float *d_points, uint32_t *d_index,
                                    uint32_t *d_counts, int capacity);
int rtuf_cloud_compact_batch_device_u16(rtuf_context *ctx, int n_streams, const uint16_t *d_depth_mm, float *d_points, uint32_t *d_index,
                                        uint32_t *d_counts, int capacity);
int rtuf_cloud_batch(rtuf_context *ctx, int n_streams, const float *const *depth_in, float *const *points_out);
int rtuf_cloud_batch_u16(rtuf_context *ctx, int n_streams, const uint16_t *const *depth_mm_in, float *const *points_out);
int rtuf_cloud_compact_batch(rtuf_context *ctx, int n_streams, const float *const *depth_in, float *const *points_out,
                             uint32_t *const *index_out, uint32_t *counts_out, int capacity);
int rtuf_cloud_compact_batch_u16(rtuf_context *ctx, int n_streams, const uint16_t *const *depth_mm_in, float *const *points_out,
                                 uint32_t *const *index_out, uint32_t *counts_out, int capacity);

/* POINT LIST BATCHES.  New, beyond the reference: filter points instead of planes -- spinning and solid-state lidars, a cloud
 * that has already been transformed or cropped, the compacted cloud this library itself emits (robot_self_filter's input).
 * A points batch renders the robot's virtual depth (VIRTUAL DEPTH) into a plane the library owns and judges every point of
 * every stream against it: a verdict byte per point, optionally the pixel it landed on, and a per-stream summary.  No sensor
 * plane is read and no image plane is returned.
 * Definition.  Every float operation is single precision and rounded on its own; divisions are IEEE.
 * Input, per stream s: count[s] points (x, y, z) in the stream's optical frame -- the frame the cloud calls write in: x right,
 * y down, z forward, pixel row 0 first.
 * Intrinsics: those of rtuf_set_cloud_intrinsics, as fx = (float)fx, fy = (float)fy, cx = (float)cx, cy = (float)cy.
 * Transform, optional and per stream: rtuf_set_point_transforms gives streams first_stream .. first_stream + n_streams - 1 one
 * column-major matrix each (optical_from_points [n][16]; NULL: none for these streams).  Its 12 used entries m are rounded to
 * float, and a point becomes p'_r = ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r], r = 0 .. 2.  A stream without a
 * transform takes its points as given, with no arithmetic at all, so an infinite coordinate does not poison the others.  The
 * setter waits for the batches in flight and applies to all pipelines, as rtuf_set_cloud_intrinsics does; an entry among the
 * 12 that is not finite (as a double or once rounded to float) or a stream range outside the context fails with
 * RTUF_ERR_INVALID and changes nothing.
 * Pixel of a point (point_pixel in rtuf_numerics.h, the inverse of cloud_point).  The point is JUDGED iff z > 0 && z < +inf
 * and both range tests below hold:
 *   a = x / z,   uf = ((a * fx) + cx) + 0.5f,      b = y / z,   vf = ((b * fy) + cy) + 0.5f
 *   uf >= 0 && uf < (float)W && vf >= 0 && vf < (float)H           (so NaN fails)
 *   u = (int)uf,  v = (int)vf
 * The range tests come before the conversions: no out-of-range float is ever converted, no index outside the plane is ever
 * formed.  Pixel centres sit at integer u, as depth_image_proc puts them: a point cloud_point made from pixel (u, v) lands on
 * (u, v) again.
 * Verdict.  V(q) is what rtuf_render_batch_device with empty_value = +inf writes at pixel q, t is
 * rtuf_params.depth_distance_threshold, r is the call's radius_px, 0 .. 4, and Vmin is the smallest V(q) over the pixels of
 * the (2r+1)^2 square around (u, v) that lie in this stream's image -- the square is never padded and never reaches into
 * another stream.  A judged point is FILTERED (verdict 1) iff z > Vmin - t, else KEPT (0); a point that is not judged is
 * OUTSIDE (2).  Where the square holds nothing drawn by a link, Vmin is +inf and the compare is false for every t: nothing is
 * special-cased.  The background quad filters nothing here (a point list has no "beyond the far plane" artefact to
 * reproduce).  to_linear_depth is monotone in the window z, so for r equal to a dilation radius the verdict is the dilated
 * filter's mask bit for a sensor plane that held z at that pixel, wherever a link, not the background, holds the minimum.
 * Layout: the compacted cloud's, so the output of rtuf_cloud_compact_batch_device can be fed straight back.  d_points is
 * [n][capacity][3] float, d_counts [n] uint32 ON THE DEVICE; stream s judges entries j < min(counts[s], capacity), and
 * everything else in d_verdict ([n][capacity] uint8) and d_pixel (NULL or [n][capacity] uint32) is left untouched.  d_pixel
 * holds v * W + u, or 0xFFFFFFFF for verdict 2.  d_summary (NULL or [n][4] uint32) holds kept, filtered, outside and
 * min(count, capacity); it is overwritten by every call and every re-run, and holds integers only, so no order of execution
 * enters.  1 <= capacity <= 1 << 24.  Alignment is the elements' own; where d_points and d_pixel start on 16-byte boundaries,
 * d_verdict on a 4-byte one and capacity is a multiple of 4, the kernel takes 16-byte loads and stores.
 * rtuf_points_batch is the host form, synchronous: points up, results down, capacity = the largest count; verdict_out and
 * pixel_out (NULL or one array per stream) receive counts[s] entries per stream, summary_out (NULL or [n][4]) the summary.
 * Refusals, each of which enqueues nothing and writes nothing.  RTUF_ERR_INVALID: a NULL d_points, d_counts or d_verdict; n,
 * capacity or radius_px out of range; and, not supported yet, silhouette_dilation_px > 0 (radius_px is this batch's own
 * margin), link padding in effect and per-link thresholds in effect.  RTUF_ERR_STATE: a context that is not finalized, or a
 * stream without intrinsics.  RTUF_FLAG_TWO_KERNEL and scene planes do not enter.
 * Otherwise it is a batch like any other: raster lanes, pipelines, launch groups, partial batches, and as many in flight as
 * render batches, each with outputs of its own (the library keeps one virtual depth plane [max_streams][H][W] per batch
 * slot, allocated on first use and counted in rtuf_stats.device_bytes); small batches replay captured graphs; a re-run after
 * a bin regrowth rewrites verdicts, pixels and summary as if the batch had run once; the status word covers the outputs
 * (the points kernel runs on each launch group's lane before its counters are published; timings: ms_compare), and
 * rtuf_order_stream_after_batches applies.
 * Out of scope: a compacted "kept points" output (which verdicts count as kept differs between one camera-like sensor and
 * several streams used as faces around a 360-degree lidar: compact on the verdict bytes); one list shared by several
 * streams; honouring padding, dilation and per-link thresholds; a ROS PointCloud2 adapter. */
int rtuf_set_point_transforms(rtuf_context *ctx, int first_stream, int n_streams, const double *optical_from_points /* [n][16] column-major, NULL = none */);
int rtuf_points_batch_device(rtuf_context *ctx, int n_streams, const float *d_points, const uint32_t *d_counts, int capacity,
                             int radius_px, uint8_t *d_verdict, uint32_t *d_pixel, uint32_t *d_summary);
int rtuf_points_batch(rtuf_context *ctx, int n_streams, const float *const *points_in, const uint32_t *counts /* host */,
                      int radius_px, uint8_t *const *verdict_out, uint32_t *const *pixel_out, uint32_t *summary_out);

/* VOXEL OCCUPANCY GRIDS.  New, beyond the reference: the kept points of ALL streams in one world grid -- which part of the
 * workspace holds something that is neither robot nor learned scene -- as a bit per voxel and, optionally, a count per voxel:
 * what a mapper, a planner's collision world or a speed-and-separation monitor asks of a cell with several cameras.  The
 * context holds one grid; inserts accumulate in it until it is cleared.
 * Definition.  Every float operation is single precision and rounded on its own.
 * Grid: rtuf_set_voxel_grid gives the origin o (3 doubles, rounded to float), voxel_size (rounded to float; inv = 1.0f /
 * voxel_size) and dims = (nx, ny, nz).  Voxel (ix, iy, iz) has index i = (iz * ny + iy) * nx + ix.  The bit grid holds bit
 * i & 31 of word i >> 5, in ceil(nx * ny * nz / 32) uint32 words; the optional count grid (with_counts != 0) one uint32 per
 * voxel, which WRAPS modulo 2^32.  Limits: each dimension 1 .. 2048, nx * ny * nz <= 1 << 27; voxel_size as a float finite
 * and > 0 with a finite inv; a finite origin (as doubles and as floats).  The call allocates and zeroes the grid (both arrays
 * in multiples of 16 bytes, counted in rtuf_stats.device_bytes); calling it again replaces the grid, dims == NULL frees it.
 * Transform, optional and per stream: rtuf_set_voxel_transforms gives streams first_stream .. first_stream + n_streams - 1 one
 * column-major matrix each (world_from_optical [n][16]; NULL: none for these streams).  Its 12 used entries m are rounded to
 * float and applied exactly as rtuf_set_point_transforms defines: p'_r = ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) +
 * m[12 + r].  A stream without one takes the point as it is, with no arithmetic.  Validation and waiting as in
 * rtuf_set_point_transforms.  The transforms outlive the grid.
 * Voxel of a world point p (voxel_of in rtuf_numerics.h): g_r = (p_r - o_r) * inv; the point is IN iff g_r >= 0 &&
 * g_r < (float)dims_r for r = 0 .. 2 -- NaN and infinities fail, nothing is special-cased, the grid's high faces are outside
 * -- and then i_r = (int)g_r.  The range tests come before the conversions, as for the pixel of a listed point.
 * Plane form (rtuf_voxel_insert_batch*).  A pixel of stream s is KEPT iff its mask bit is 0 and its sensor value carries a
 * point (positive and finite, as the cloud calls define it).  The mask bit is that of the mask-bits batch the context would
 * run on these planes: dilation, per-link thresholds, link padding and scene planes are honoured.  The pixel's point is that of
 * the cloud calls (cloud_point with the intrinsics of rtuf_set_cloud_intrinsics), then the stream's transform.  Every kept
 * pixel whose voxel is IN sets that voxel's bit and adds 1 to its count.
 * Point-list form (rtuf_voxel_insert_points_device).  The layout is that of rtuf_points_batch_device: d_points
 * [n][capacity][3], d_counts [n] on the device, entries j < min(count, capacity).  An entry is taken iff d_verdict is NULL or
 * its verdict byte is 0 (kept).  Its point first goes through the stream's point transform (rtuf_set_point_transforms, if set),
 * then through world_from_optical.  So a compacted cloud, and a lidar list judged by a points batch, are inserted as they are.
 * 16-byte loads where the points batch's alignment rule holds (d_verdict, if given, on a 4-byte boundary).
 * Summary: d_summary is NULL or [n][4] uint32 per call -- inserted, outside the grid, not kept, total (H * W for the plane
 * form, min(count, capacity) for the list form).  Every call overwrites it.  Bits are ORed and counts are added: everything is
 * an integer, so no order of execution enters any output.
 * Order of an insert.  It is synchronous, as learning a scene is, because an OR cannot be taken back: everything in flight is
 * retired; the plane form then runs a mask-bits batch into a buffer of the context and retires it INCLUDING its re-run after
 * a bin regrowth, so provisional bits never reach the grid; then one kernel runs and is waited for.  The list form retires
 * what is in flight because its input may be a batch's output.  With several pipelines the grid lives in the first one and
 * inserts run there, as rtuf_learn_scene_batch* does.
 * rtuf_voxel_clear zeroes bits and counts.  rtuf_voxel_grid_device hands out the device arrays (any of the three out-pointers
 * may be NULL; valid until the grid is replaced or freed), rtuf_get_voxel_grid copies them to the host (either may be NULL).
 * Errors, each of which writes nothing and changes no grid.  RTUF_ERR_INVALID: bad arguments (a NULL array, n, capacity, dims,
 * size or origin out of range), and the mask-bits calls' refusals with their texts (plane form: among them a width that is
 * not a multiple of 4, 32FC1 and 16UC1 alike; the list form and rtuf_voxel_carve_batch* take any width).  RTUF_ERR_STATE: no grid, a
 * context that is not finalized, a stream without cloud intrinsics (plane form), a count grid asked for -- counts_out, or the
 * d_counts out-pointer -- when the grid has none.
 * Out of scope: log-odds or decay, a threshold on counts, an asynchronous insert, merging
 * the grids of several GPUs (OR the bit words, add the counts), a ROS OccupancyGrid or octomap adapter, labels per voxel. */
int rtuf_set_voxel_grid(rtuf_context *ctx, const double origin[3], double voxel_size, const int dims[3], int with_counts);
int rtuf_set_voxel_transforms(rtuf_context *ctx, int first_stream, int n_streams, const double *world_from_optical /* [n][16] column-major, NULL = none */);
int rtuf_voxel_clear(rtuf_context *ctx);
int rtuf_voxel_insert_batch(rtuf_context *ctx, int n_streams, const float *const *depth_in, uint32_t *summary_out);
int rtuf_voxel_insert_batch_u16(rtuf_context *ctx, int n_streams, const uint16_t *const *depth_mm_in, uint32_t *summary_out);
int rtuf_voxel_insert_batch_device(rtuf_context *ctx, int n_streams, const float *d_depth, uint32_t *d_summary);
int rtuf_voxel_insert_batch_device_u16(rtuf_context *ctx, int n_streams, const uint16_t *d_depth, uint32_t *d_summary);
int rtuf_voxel_insert_points_device(rtuf_context *ctx, int n_streams, const float *d_points, const uint32_t *d_counts, int capacity,
                                    const uint8_t *d_verdict, uint32_t *d_summary);
int rtuf_voxel_grid_device(rtuf_context *ctx, const uint32_t **d_bits, const uint32_t **d_counts, size_t *n_voxels);
int rtuf_get_voxel_grid(rtuf_context *ctx, uint32_t *bits_out, uint32_t *counts_out);

/* VOXEL FREE SPACE.  New, beyond the reference: the third state of the grid above.  A clear occupancy bit is ambiguous: a
 * camera may have looked THROUGH the voxel and seen further, or no camera can see the voxel at all -- behind the robot, behind
 * an intruder, outside every frustum, a sensor hole.  A carve marks the first kind in a second bit array, the FREE grid.
 * Reading: occupied wins; free and not occupied = seen through; neither = unknown, which a speed-and-separation monitor must
 * treat as occupied and a planner must not drive through.  It is built projectively, voxel by voxel, not ray by ray: every
 * voxel centre is projected into every stream's sensor plane and compared with what the sensor read there.
 * Definition.  Every float operation is single precision and rounded on its own; divisions are IEEE.
 * Free grid: a second bit array beside the occupancy bits with the same indexing (bit i & 31 of word i >> 5), allocated in
 * multiples of 16 bytes and zeroed on the first carve or the first read and counted in rtuf_stats.device_bytes.
 * rtuf_voxel_clear zeroes it too; rtuf_set_voxel_grid frees it with the grid, whether the grid is replaced or dims == NULL.
 * Bits are ORed over calls, as inserts are.  Bits at indices >= nx * ny * nz are always 0.
 * Voxel centre (voxel_centre in rtuf_numerics.h): size = (float)voxel_size, c_r = o_r + ((float)i_r + 0.5f) * size -- one add
 * (exact), one product, one add.
 * Into the optical frame: a stream without a voxel transform takes the centre as it is, with no arithmetic; a stream with one
 * takes it through optical_from_world, the inverse of the 12 FLOATS the insert uses, computed on the host in double
 * (voxel_inverse_transform): a(r,c) the floats as doubles, the nine cofactors each p * q - r * s, det = (a00 C00 + a01 C01) +
 * a02 C02, R = adj / det with one division per entry, t'_r = -((R_r0 t_0 + R_r1 t_1) + R_r2 t_2), each of the 12 results then
 * rounded to float, and applied exactly as rtuf_set_point_transforms defines.  The table is rebuilt whenever
 * rtuf_set_voxel_transforms changes a stream.  A stream whose det is 0 or not finite, or one of whose 12 results is not finite
 * as a float, cannot be carved from (see Errors); inserts are not affected.
 * Pixel: that of a listed point (point_pixel as it stands: z > 0 && z < inf, the range tests before the conversions) with the
 * intrinsics of rtuf_set_cloud_intrinsics.  A centre that is not judged is NOT SEEN by that stream.
 * Free test: s(q) is the sensor value at pixel q (32FC1: the float; 16UC1: float(u16) * 0.001f, as the cloud calls define it),
 * valid(q) iff it carries a point (positive and finite).  radius_px = r, 0 .. 4: Emin is the smallest s(q) over the VALID
 * pixels of the (2r + 1)^2 square around (u, v) that lie in this stream's image -- never padded, never in another stream;
 * invalid neighbours are skipped: an absent ray says nothing.  m = (float)margin.  The voxel is FREE for the stream iff the
 * centre is judged, the centre pixel is valid and z < Emin - m (one subtraction); NOT FREE iff it is judged and not free.
 * The mask is NOT read: the space in front of the robot's surface is free, what lies behind it fails z < s by itself, so the
 * robot's own volume stays unknown.  margin is along the optical axis; at least half the voxel diagonal (0.87 voxel_size) is
 * recommended, so that a voxel is only freed when all of it lies in front of the reading.
 * Output: the free bit of voxel i is ORed with "FREE for at least one of the n streams".  d_summary is NULL or [n][4] uint32
 * per call -- free, not free, not seen, nx * ny * nz -- overwritten by every call.  Integers and one owner per output word: no
 * order of execution enters any output.
 * A voxel may be both occupied and free: a point fell into it, yet its centre projects onto a pixel that reads deeper -- an
 * edge, a slanted surface, another camera.  Both bits stand; occupied wins.
 * Order: a carve is synchronous, like an insert: everything in flight is retired (the planes may be a batch's output), then one
 * kernel runs on the first pipeline and is waited for.  It is no batch kind.  The sensor planes are only read.  Any image width
 * is accepted: no mask-bits batch runs.
 * rtuf_voxel_free_device hands out the device array (either out-pointer may be NULL; valid until the grid is replaced or
 * freed), rtuf_get_voxel_free copies its ceil(nx * ny * nz / 32) words to the host.
 * Errors, each of which writes nothing and changes no grid.  RTUF_ERR_INVALID: a NULL plane array or a NULL plane in it, n
 * outside 1 .. max_streams, radius_px outside 0 .. 4, a margin that is negative or not finite (as a double or as a float), a
 * stream among the n whose transform cannot be inverted (the message names the stream).  RTUF_ERR_STATE: no grid, a context
 * that is not finalized, a stream among the n without cloud intrinsics.
 * Out of scope: clearing occupied bits along the rays, log-odds, decay; a pixel radius that follows the voxel's projected
 * size; treating "no return" as free up to a maximum range; marking the robot's own volume from the virtual depth; a count of
 * seeing cameras per voxel; carving from point lists; an asynchronous carve; merging several GPUs' grids (OR the words). */
int rtuf_voxel_carve_batch_device(rtuf_context *ctx, int n_streams, const float *d_depth, double margin, int radius_px, uint32_t *d_summary);
int rtuf_voxel_carve_batch_device_u16(rtuf_context *ctx, int n_streams, const uint16_t *d_depth_mm, double margin, int radius_px, uint32_t *d_summary);
int rtuf_voxel_carve_batch(rtuf_context *ctx, int n_streams, const float *const *depth_in, double margin, int radius_px, uint32_t *summary_out);
int rtuf_voxel_carve_batch_u16(rtuf_context *ctx, int n_streams, const uint16_t *const *depth_mm_in, double margin, int radius_px, uint32_t *summary_out);
int rtuf_voxel_free_device(rtuf_context *ctx, const uint32_t **d_free_bits, size_t *n_voxels);
int rtuf_get_voxel_free(rtuf_context *ctx, uint32_t *free_out);

/* LINK CLEARANCE TABLES.  New, beyond the reference: per stream and link label, how close the nearest kept point -- the
 * nearest thing that is not the robot -- is to the link, as a table [n_streams][n_labels] of 16-byte rows with no plane
 * written at all: what speed-and-separation monitors and reactive controllers ask of the filtered cloud.
 * Spheres.  rtuf_set_link_spheres gives `model` its list: sphere i is attached to link link[i] of the model, its centre
 * xyzr[i][0..2] is in the link's frame -- the frame rtuf_set_link_poses places, in which a draw's vertices stand once its
 * pre_op (glScalef / glTranslatef) has been applied to them: no pre_op is ever applied to a sphere, so a caller that derives
 * spheres from a draw's vertices scales or translates those vertices first -- and its radius xyzr[i][3] is >= 0.
 * Callable after rtuf_finalize_models, between batches (it waits for the batches in flight); it replaces the model's list,
 * n_spheres = 0 clears it.  More than 4096 spheres in the context, more than 256 distinct non-zero labels among them, a bad
 * link index, a non-finite centre or a negative or non-finite radius fail with RTUF_ERR_INVALID and change nothing.  A sphere
 * takes the label of its link (LINK LABELS: default labels or rtuf_set_link_labels) when a batch is enqueued -- a batch after
 * a relabelling that leaves more than 256 labels fails with RTUF_ERR_INVALID -- and spheres of label 0 are ignored.  Spheres
 * have a context-global id: model order, then list order (ignored spheres keep theirs).
 * A kept point is the cloud batch's (FILTERED POINT CLOUDS): mask bit 0 -- silhouette dilation and per-link thresholds
 * honoured -- and sensor > 0 && sensor < +inf; the point is cloud_point with the stream's rtuf_set_cloud_intrinsics.
 * A sphere's centre in the camera frame is offset_inv * (cam_tf * (link_tf[stream][link] * (c, 1))): three matrix-vector
 * products in double, every row ((m0 x + m4 y) + m8 z) + m12 with each product and sum rounded on its own, the result rounded
 * to float (clearance_centre in rtuf_numerics.h).  That is the cloud's optical frame: the reference applies its look-at after
 * camera_offset_inv.  The clearance of a (point, sphere) pair is sqrt((dx dx + dy dy) + dz dz) - r, d = point - centre, in
 * single float operations with a correctly rounded square root (clearance_point_sphere); it is negative inside the sphere.
 * A pair COUNTS iff clearance < max_distance, strictly; max_distance > 0, +inf allowed (NaN or <= 0: RTUF_ERR_INVALID).
 * Row l >= 1 of stream s, over the spheres of label l of the models the stream renders (rtuf_set_stream_models):
 * points_within = the kept points with a counting pair; clearance / pixel / sphere = the counting pair with the smallest
 * clearance, then the smallest pixel index v * width + u, then the smallest sphere id; {+inf, 0xFFFFFFFF, 0xFFFFFFFF, 0} when
 * no pair counts (also: no spheres of that label).  Row 0 is the whole robot: the same over the spheres of all labels
 * 1 .. n_labels - 1 together, so its points_within is not the sum of the other rows.  Spheres of labels >= n_labels are
 * dropped, from row 0 too.  Every call overwrites its table.  Minima and integer counts only: the table does not depend on
 * the order of execution, and the kernels' culling is conservative -- the result is that of all pairs.
 * A clearance batch is a mask-bits batch plus the clearance kernels, as a cloud batch is, with the cloud batch's rules --
 * the library's own bits buffer per batch slot (and the posed spheres), RTUF_FLAG_TWO_KERNEL does not enter, thresholds not
 * together with dilation (RTUF_ERR_INVALID), a stream without intrinsics fails with RTUF_ERR_STATE, an uncovered image makes
 * retiring the batch fail with RTUF_ERR_STATE -- except that any width is accepted, 16UC1 included.  Otherwise it is a batch
 * like any other: raster lanes, pipelines, launch groups, partial batches, batches in flight (each with a table of its own),
 * graph replay of small batches, re-runs after a bin regrowth (the rows start over: as if the batch had run once), the status
 * word, which covers the table (timings: ms_compare), rtuf_order_stream_after_batches.  The device forms only enqueue
 * (d_table: [n][n_labels], 8-byte aligned); the host-plane forms are synchronous: planes up, table down.  n_labels < 1, a
 * NULL plane or table, n out of range or an un-finalized context fail as the filter calls do; a refused call enqueues nothing. */
int rtuf_set_link_spheres(rtuf_context *ctx, int model, const int32_t *link /* [n] */, const float *xyzr /* [n][4] */, int n_spheres);
typedef struct {
  float clearance;        /* metres, may be negative (point inside a sphere); +inf: nothing within max_distance          */
  uint32_t pixel;         /* v * width + u of the nearest kept pixel; 0xFFFFFFFF when clearance is +inf                  */
  uint32_t sphere;        /* context-global id of the sphere it is nearest to; 0xFFFFFFFF likewise                       */
  uint32_t points_within; /* kept points whose clearance to this label's spheres is < max_distance                       */
} rtuf_link_clearance;    /* 16 bytes */

int rtuf_link_clearance_batch_device(rtuf_context *ctx, int n_streams, const float *d_depth, rtuf_link_clearance *d_table, int n_labels,
                                     float max_distance);
int rtuf_link_clearance_batch_device_u16(rtuf_context *ctx, int n_streams, const uint16_t *d_depth_mm, rtuf_link_clearance *d_table, int n_labels,
                                         float max_distance);
int rtuf_link_clearance_batch(rtuf_context *ctx, int n_streams, const float *const *depth_in, rtuf_link_clearance *table_out, int n_labels,
                              float max_distance);
int rtuf_link_clearance_batch_u16(rtuf_context *ctx, int n_streams, const uint16_t *const *depth_mm_in, rtuf_link_clearance *table_out,
                                  int n_labels, float max_distance);

/* LINK PADDING.  New, beyond the reference: a margin in metres around every link's silhouette, per link -- what
 * robot_self_filter's padding and MoveIt's padding_offset give.  rtuf_set_link_thresholds pads a link ALONG the ray;
 * silhouette_dilation_px pads across it, but by one radius in pixels for the whole image.  Padding is across the ray, metric
 * and per link: a drawn pixel of link g at depth d spreads its depth over the disc of pad[g] * f / d pixels around it, the
 * projection of a ball of pad[g] metres at that depth, so the margin shrinks with distance as the robot's image does.
 * Definition (every float operation single precision and rounded on its own), per stream:
 *   f      = (float)max(fx, fy) of rtuf_set_cloud_intrinsics (the larger one: the margin is never under-stated)
 *   Z(q)   = the window z of the fragment that won pixel q (GL_LESS on the 24-bit depth, ties to the earlier draw), NaN where
 *            nothing was drawn
 *   S(q)   = 0 where the background quad won or nothing was drawn, else 1 + the context-global number of the winner's link
 *   pad[s] = the padding of the link of slot s in metres, pad[0] = 0
 *   d(q)   = num / (Z(q) - off)                   the shader's to_linear_depth, IEEE division
 *   rho    = fminf((pad[S(q)] * f) / d(q), 16)    product, then IEEE division; 16 = RTUF_MAX_LINK_PADDING_PX
 *   R2(q)  = (uint32_t)(rho * rho)                truncated; 0 where Z(q) is NaN, S(q) is 0 or the pad is 0
 *   z'(p)  = the smallest Z(q) over the pixels q of the image with Z(q) not NaN and (px-qx)^2 + (py-qy)^2 <= R2(q), in
 *            integers; NaN when there is none.  p itself always qualifies when it is drawn.
 * and pixel p is shaded as silhouette dilation shades: the global depth_distance_threshold against z'(p), the GL clear colour
 * where z'(p) is NaN (for mask bits: the "uncovered" state).  z' is a minimum of input values: no order of execution enters.
 * THE CLAMP at RTUF_MAX_LINK_PADDING_PX = 16 pixels is part of the definition: nearer than d = pad * f / 16 the margin stops
 * growing in the image -- a 2 cm margin reaches 16 pixels at d = f / 800 (0.66 m at f = 525).
 * rtuf_set_link_padding sets the paddings of one model's links (n_links = rtuf_num_links(model)), each finite and >= 0;
 * rtuf_clear_link_padding removes them.  Both wait for the batches in flight and take effect with the next batch enqueued; a
 * bad model id, a wrong n_links, a NULL array, a negative, NaN or infinite value, or a context of more than 65,534 links fail
 * with RTUF_ERR_INVALID and change nothing.  The draw-order -> slot table (2 bytes per triangle) and the slot -> padding table
 * are allocated by the first rtuf_set_link_padding, a 2-byte slot plane per lane and stream of the launch group by the first
 * padded batch.
 * Padding is IN EFFECT while some model holds a non-zero value.  Then
 *   - every filter batch (device, host-plane, asynchronous, f32 and 16UC1), mask-bits batch, cloud batch and clearance batch
 *     honours it -- so filtered point clouds and link clearance tables hold neither the robot nor its halo.  They all take the
 *     z-surface route whatever RTUF_FLAG_TWO_KERNEL says (the mask-bits calls still refuse that flag), one batch in flight at a
 *     time, as with dilation;
 *   - the link label calls, render batches, residual batches, any batch with silhouette_dilation_px > 0 and any batch while
 *     per-link thresholds are in effect (equal depths of two links would make "the winner's threshold" ambiguous) fail with
 *     RTUF_ERR_INVALID before anything is enqueued: not supported yet;
 *   - a batch with a stream that has no intrinsics fails with RTUF_ERR_STATE.
 * While it is not -- after the last rtuf_clear_link_padding too -- nothing differs from a context that never used it: batches
 * take the routes and kernels they always took. */
#define RTUF_MAX_LINK_PADDING_PX 16
int rtuf_set_link_padding(rtuf_context *ctx, int model, const float *padding_m, int n_links);
int rtuf_clear_link_padding(rtuf_context *ctx, int model);

/* SCENE PLANES.  New, beyond the reference: also filter the static scene -- the pedestal, the table, the fence, the floor --
 * from a per-stream depth plane of the empty cell, which can be set or LEARNED from the camera's own frames while the robot
 * moves in front of it.  With a scene in effect a link clearance table measures the distance from the robot to an intruder, not
 * to the table, and a filtered point cloud holds only what is new in the cell.  ("Background" already names the far-plane quad
 * here; this is the scene.)
 * Per stream the context holds one float plane scene[H][W] in metres, whatever the element type of the batches; every pixel
 * is +inf until it is set or learned, and +inf and NaN mean "unknown".  It also holds two margins, abs_m >= 0 and rel in
 * [0, 1), and a switch.  Definition (every float operation single precision and rounded on its own), per pixel p:
 *   thr(p)            = scene(p) - (abs_m + rel * scene(p))
 *   scene_filtered(p) = s(p) > thr(p)         s: the sensor value in metres (16UC1: float(u) * 0.001f, as everywhere)
 * The comparison is strict and ordered: a NaN sensor value is never scene-filtered, and an unknown scene pixel never filters
 * anything (thr is NaN for every legal margin; nothing is special-cased).  For a stream whose scene filtering is
 * enabled
 *   filtered(p) = the robot filter's verdict (exactly today's, with dilation, thresholds and padding as configured)
 *                 OR scene_filtered(p)
 *   masked(p)   = filtered(p) ? filter_replace_value : sensor(p)     (16UC1: the value the robot filter writes there)
 * in every filter batch (device, host-plane, asynchronous, f32 and 16UC1, with or without a byte mask or a label plane),
 * mask-bits batch, cloud batch and clearance batch; mask byte 255 and mask bit 1 mean filtered, as ever.  Label planes are
 * untouched (a scene-filtered pixel no link won keeps label 0); render and residual batches compare nothing against the
 * scene.  Nothing is refused because of a scene: labels, RTUF_FLAG_TWO_KERNEL, dilation, thresholds and padding keep working.
 * A masked plane that aliases the sensor plane stays legal wherever it is today.
 *   rtuf_set_scene_planes / _device   set the planes of streams first_stream .. first_stream + n_streams - 1 from n_streams
 *                                     host pointers / one packed device array [n_streams][H][W]; any float value is accepted
 *   rtuf_get_scene_planes / _device   read them back (+inf everywhere for a context that never held a scene)
 *   rtuf_set_scene_margins            abs_rel = [n_streams][2] {abs_m, rel}: sets the margins and ENABLES scene filtering for
 *                                     those streams; NULL disables it for them and keeps their planes and margins
 *   rtuf_clear_scene                  disables filtering, resets the planes to +inf and the margins to 0
 *   rtuf_learn_scene_batch*           streams 0 .. n_streams - 1: for every pixel the ROBOT filter keeps (its bits honour
 *                                     dilation, thresholds and padding, never the scene) and whose reading carries a point
 *                                     (positive and finite), scene = min(scene, s); a NaN scene value counts as unknown and is
 *                                     replaced.  Every other pixel is left alone; no output plane is written.  Learn with link
 *                                     padding on, so that the arm's halo is not learned.  A running minimum of input values:
 *                                     idempotent, and independent of the frames' order.
 * The setters wait for the batches in flight and take effect with the next batch enqueued, like rtuf_set_link_padding.  The
 * learn calls are a calibration phase, not the hot path: they are synchronous -- they wait for the batches in flight, run a
 * mask-bits batch into a buffer of the context, let the host retire it INCLUDING its re-run after a bin overflow, and only
 * then update the planes, so provisional bits never reach them.  They inherit the mask-bits calls' conditions (a width that
 * is a multiple of 4, the background quad covers the image, RTUF_FLAG_TWO_KERNEL refused) and report them the same way.
 * A stream range outside 0 .. max_streams, a NULL plane or array, a negative, NaN or infinite margin or rel >= 1 fail with
 * RTUF_ERR_INVALID and change nothing; a context that is not finalized fails with RTUF_ERR_STATE.  The planes (max_streams *
 * H * W * 4 bytes), the streams' table and learning's scratch are allocated by the first call that needs them and counted in
 * rtuf_stats.device_bytes.
 * A scene is IN EFFECT in the context while some stream has filtering enabled: then every batch of the kinds above runs one
 * more streaming kernel per launch group (scene_apply_planes_kernel or scene_apply_bits_kernel), which
 * skips the streams that have it disabled.  While none has -- and after rtuf_clear_scene cleared the last stream that was ever
 * touched, when the memory is returned too -- nothing differs from a context that never used a scene. */
int rtuf_set_scene_planes(rtuf_context *ctx, int first_stream, int n_streams, const float *const *planes);
int rtuf_set_scene_planes_device(rtuf_context *ctx, int first_stream, int n_streams, const float *d_planes);
int rtuf_get_scene_planes(rtuf_context *ctx, int first_stream, int n_streams, float *const *out);
int rtuf_get_scene_planes_device(rtuf_context *ctx, int first_stream, int n_streams, float *d_out);
int rtuf_set_scene_margins(rtuf_context *ctx, int first_stream, int n_streams, const float *abs_rel);
int rtuf_clear_scene(rtuf_context *ctx, int first_stream, int n_streams);
int rtuf_learn_scene_batch(rtuf_context *ctx, int n_streams, const float *const *depth_in);
int rtuf_learn_scene_batch_u16(rtuf_context *ctx, int n_streams, const uint16_t *const *depth_mm_in);
int rtuf_learn_scene_batch_device(rtuf_context *ctx, int n_streams, const float *d_depth);
int rtuf_learn_scene_batch_device_u16(rtuf_context *ctx, int n_streams, const uint16_t *d_depth);

/* Counters of the last batch and kernel timings measured with HIP events on the context's
 * stream (replaces the wall-clock statistics of src/urdf_filter.cpp:239-266). */
typedef struct {
  uint64_t triangles_submitted;     /* triangles x streams handed to set-up            */
  uint64_t triangles_binned;        /* (sub-)triangles that reached at least one tile  */
  uint64_t bin_entries;             /* records written to tile bins                    */
  uint64_t triangles_clipped;       /* triangles that went through the clipper         */
  uint32_t max_bin_fill;            /* largest bin of the last batch                   */
  uint32_t bin_capacity;
  uint32_t regrowths;               /* times the bins were enlarged and a batch re-run */
  uint32_t max_fbin_fill;           /* largest fragment bin of the last batch          */
  uint64_t fragments_binned;        /* covered pixels of small (<= 4x4 px box) triangles binned as fragments */
  float ms_pose, ms_setup, ms_raster, ms_compare, ms_total;   /* last timed batch       */
  float ms_clip;                    /* clip kernel alone (timing modes 2 / 3; in mode 1 it is part of ms_setup) */
  uint64_t timed_batches;           /* batches retired since rtuf_enable_timing, and the sums  */
  double sum_ms_pose, sum_ms_setup, sum_ms_raster, sum_ms_compare, sum_ms_total;   /* of their times */
  double sum_ms_clip;
  /* ABI 4 */
  uint64_t device_bytes;            /* device memory the context holds right now (all pipelines)                      */
  uint64_t occluded_entries;        /* (record, tile) pairs never appended: they lie behind a triangle that covers the tile */
  uint32_t cover_tiles;             /* tiles whose initial depth keys came from a triangle covering the whole tile     */
  uint32_t exact_tiles;             /* tiles that ran the exact-z pass (a winner with window z <= 0.5)                 */
  uint32_t work_items;              /* set-up work items (chunk x up to 3 streams that see it) of the last batch       */
  uint32_t zero_survivor_items;     /* ... of which no triangle survived the clip / sub-pixel culls                    */
  uint32_t cover_pass;              /* 1: the last batch ran the cover pass (on while scenes have whole-tile triangles,
                                       switched off after three batches without one, probed again every 64th batch)     */
  uint32_t counter_blocks;          /* counter blocks of each batch slot: the most launch groups any batch of 1 .. max_streams
                                       streams can be split into at the present launch group (was reserved0; a batch of fewer
                                       streams than max_streams can need more groups than a full one)                    */
  uint64_t raster_atomics;          /* instrumented builds (-DRTUF_COUNT) only: depth tests the tile kernel issued      */
  uint64_t drawn_pixels;            /* instrumented builds only: pixels whose final depth key is not the background's   */
  /* ABI 5 */
  uint32_t raster_lanes;            /* raster lanes of the context (of each pipeline)                                   */
  uint32_t launch_group;            /* streams a lane's bins are sized for right now (shrinks when memory is short)      */
  uint32_t groups_last_batch;       /* launch groups the last batch was split into                                       */
  uint32_t graphs_enabled;          /* 1 while small batches replay captured hipGraphs (pipeline children only); the library
                                       switches them off for good when captures keep evicting live entries               */
  uint64_t graph_hits, graph_misses;/* replays / captures so far                                                          */
  uint32_t lanes_side_by_side;      /* 1: the lanes' HIP streams and the pose stage's stream were measured to execute side by
                                       side at rtuf_create (with one lane: the lane's and the pose stage's).  0: every stream the
                                       runtime handed out shared a hardware queue with one of them -- everything then works, one
                                       kernel after the other; raise GPU_MAX_HW_QUEUES (HIP runtime, default 4)  */
  /* ABI 6 */
  uint32_t batch_status;            /* RTUF_STATUS_* bits the FIRST run of the batch retired last left in its device status word
                                       (0: its planes were final as soon as its kernels had run).  A batch that was run again only
                                       because an OLDER batch in flight overflowed is retired on its re-run's counters: its mirror
                                       then reads what that run left (0, batch_reruns 0) although a device-side consumer saw the
                                       first run's word -- the device word, not this mirror, is what such a consumer goes by       */
  uint32_t batch_reruns;            /* times that batch (and everything in flight behind it) was run again before it was retired */
  uint32_t over_memory_limit;       /* 1: the tile bins exceed rtuf_params.memory_limit_mb (or the automatic third of the free
                                       memory): one stream's bins alone are larger, and launch groups cannot shrink below one   */
  uint32_t copy_streams_side_by_side;  /* host-plane calls: 1 once the upload and download streams were measured to run beside the
                                       raster lanes' (first such call), 0 before that or when they share a hardware queue with a lane
                                       (copies then wait behind that lane's kernels).  RTUF_QUEUE_PROBE=0 in the environment skips
                                       all of these measurements (rtuf_create is ~10 ms faster, the flags then read 1 unmeasured)  */
} rtuf_stats;
int rtuf_get_stats(rtuf_context *ctx, rtuf_stats *out);
/* Per-kernel HIP-event timing (off by default: every event costs a few microseconds of stream
 * time).  on = 1: every stage (ms_pose, ms_setup = cull .. clip, ms_raster, ms_compare, ms_total);  on = 2: the
 * raster stage's kernels one by one: ms_setup (set-up kernel), ms_clip (clip kernel), ms_raster (tile kernel),
 * ms_compare (two-kernel mode);  on = 3: as 2, but only every eighth batch is timed (timed_batches and the sums
 * count those). */
int rtuf_enable_timing(rtuf_context *ctx, int on);

/* Debug / test access: copy the z-surface of the last batch (float window z of the winning
 * fragment per pixel, [n][H][W]) to the host.  Only valid with RTUF_FLAG_TWO_KERNEL. */
int rtuf_debug_read_zsurface(rtuf_context *ctx, int n_streams, float *host_out);

#ifdef __cplusplus
}
#endif
#endif /* RTUF_H_ */
