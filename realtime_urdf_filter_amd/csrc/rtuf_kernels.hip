// rtuf_kernels.hip -- hand-written HIP kernels (gfx950 / CDNA4, wave64) of the depth self-filter.
//
// Pipeline per batch of camera streams (pose stage on a side stream, raster stage on the main stream):
//   fk_tree_kernel  joint positions -> link matrices + camera transform   replaces urdf_renderer.cpp:173-190 (TF lookups)
//   pose_kernel     float32 OpenGL matrix stack per (stream, draw);       replaces urdf_filter.cpp:576-614,
//                   per-stream background plane; zeroes the counters      renderable.cpp:59-68, :95, :128, :427
//   cull_kernel     chunk bounding boxes vs every stream's frustum ->     (none: GL draws everything)
//                   compact work list of (chunk, 3 streams) items
//   setup_kernel    per item: vertex transform once per chunk vertex,     replaces urdf_filter.vert + the GL
//                   clip test, viewport, 1/256-px snap, sub-pixel cull,   driver's primitive assembly / set-up
//                   z plane; small boxes -> 8-B fragments, others ->
//                   32-B records, binned per 64x32 tile
//   clip_kernel     the few triangles that cross a frustum plane:         (GL driver clipper)
//                   Sutherland-Hodgman in clip space, fan, same set-up
//   bigrec_kernel   one wave per record that touches more than 4 tiles:   (binning: no counterpart in the reference)
//                   appends it to the bins of the tiles it really touches
//   tile_kernel     one workgroup per (stream, 64x32 tile): the tile's    replaces GL rasterisation + 24-bit
//                   depth keys live in LDS, fragments resolve with        GL_LESS depth test + urdf_filter.frag
//                   64-bit LDS atomicMin, then the per-pixel compare      + glGetTexImage conversions
//                   is done in place (fused) or the z-surface is written
//   compare_kernel  two-kernel mode only: z-surface + sensor -> outputs   replaces urdf_filter.frag:19-36
//   dilate_compare_kernel  silhouette dilation only (new, beyond the       (none: the reference has no dilation)
//                   reference): (2r+1)^2 window minimum of the z-surface,
//                   then compare_kernel's shading (or the mask bits)
//   pad_compare_kernel  link padding only (new as well): every drawn        (none: the reference has no padding)
//                   pixel spreads its z over the disc its link's padding
//                   projects to; the smallest z that reaches a pixel,
//                   then compare_kernel's shading (or the mask bits)
//
// Exactness: results must equal the reference's GLSL running on Mesa llvmpipe bit for bit
// (see oracle/rtuf_oracle.c for what that pins).  Every float operation whose rounding matters
// is an explicit __f*_rn intrinsic, and the file is built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "rtuf_device.h"
#include "rtuf_numerics.h"
#include "rtuf_routes.h"

namespace rtuf {

// Lane-utilisation builds (-DRTUF_LANECOUNT, scripts/lane_util.sh; never the product): every instrumented loop counts, per
// trip of a wave, 64 lane slots and the lanes for which `pred` holds (of those the hardware has active at that point) in two
// LDS words per workgroup, summed into the batch's counters when the workgroup ends.  In the product the macros are empty.
enum {
  kLaneTileLoad = 0,      // tile kernel: a wave's load + unpack of up to 64 bin records (live: lanes that hold one)
  kLaneWalkTrip,          // lane-per-triangle walk: quad trips (live: lanes whose box still has quads)
  kLaneWalkFrag,          // ... depth-test bodies the walk executed (live: lanes whose candidate is covered)
  kLaneQuarterTrip,       // quarter-wave walk: pair trips
  kLaneQuarterFrag,
  kLaneWaveTrip,          // whole-wave walk of one record (huge boxes that stay with their wave)
  kLaneWaveFrag,
  kLaneParkTrip,          // workgroup-cooperative walks of the parked records
  kLaneParkFrag,
  kLaneFragList,          // fragment list: one depth test per 8-byte fragment
  kLaneResolve,           // resolve passes (4 pixels per lane)
  kLaneSetupVert,         // set-up kernel: phase 1, a vertex per lane
  kLaneSetupTri,          // phase 2, a triangle per lane
  kLaneSetupSmall,        // phase 3a/b trips: coverage of the <= 4x4 boxes (live: lanes with a triangle)
  kLaneSetupSmallHit,     // ... of which cover a pixel centre (z plane + emission)
  kLaneSetupFragStore,    // fragment emission: per-lane store loop (trips until the lane with most covered pixels is done)
  kLaneSetupFragGroup,    // fragment emission: group-finding trips (one per distinct bin of the wave)
  kLaneSetupRec,          // phase 3c trips: set-up of the records (live: lanes with a triangle)
  kLaneSetupRecHit,       // ... of which survive orientation / bounding
  kLaneSetupRecTile,      // record emission: trips over the tiles a record touches
  kLaneSetupRecGroup,     // record emission: group-finding trips
  kLaneCount,
  // histogram of the tile kernel's bin records (live = records): by quad trips of the lane-per-triangle walk (1, 2, 3, 4, 5, 6,
  // 7-8, 9-12, 13-16, 17-24, 25+), quarter-wave class, larger, nothing in this tile; and how many records have a WHOLE box of
  // at most 8 x 8 / 8 x 4 (or 4 x 8) pixel centres inside one tile (what a larger fragment class of the set-up kernel would take)
  kLaneHist = 24, kLaneHistQuarter = kLaneHist + 11, kLaneHistLarge, kLaneHistNone, kLaneHist8x8, kLaneHist8x4, kLaneHistEnd,
  // the same two set-up loops again, counting only the trips of waves that hold a live lane at all (RTUF_LANES_LIVE: a wave
  // without one skips the body and costs next to nothing, but fills the counts above with empty slots)
  kLaneSetupVertLive = kLaneHistEnd, kLaneSetupSmallLive, kLaneEnd
};
static_assert(kLaneEnd <= kLaneLoops, "CounterShard holds kLaneLoops pairs");
static_assert(kLaneHistEnd <= kLaneLoops, "CounterShard holds kLaneLoops pairs");
static_assert(kLaneCount <= kLaneLoops, "CounterShard holds kLaneLoops pairs");
#ifdef RTUF_LANECOUNT
// LDS words of the instrumented build: 2 per loop (slots, live) and 4 per loop (trips with a live lane, by the wave's index in
// its workgroup modulo 4: the share of every loop's work that a wave gets follows from it, all loops index as base + tid)
__device__ __forceinline__ uint32_t* lane_words() { __shared__ uint32_t s_lw[6 * kLaneLoops]; return s_lw; }
__device__ __forceinline__ uint32_t lane_role() { return (threadIdx.x >> 6) & 3u; }
#define RTUF_LANES(id, pred)                                                                                          \
  do {                                                                                                                \
    const unsigned long long act_ = __ballot(true), m_ = __ballot(pred);                                              \
    if ((int)(threadIdx.x & 63) == __ffsll((long long)act_) - 1) {                                                    \
      atomicAdd(&lane_words()[2 * (id)], 64u);                                                                        \
      atomicAdd(&lane_words()[2 * (id) + 1], (uint32_t)__popcll(m_));                                                 \
      if (m_) atomicAdd(&lane_words()[2 * kLaneLoops + 4 * (id) + lane_role()], 1u);                                  \
    }                                                                                                                 \
  } while (0)
#define RTUF_LANES_LIVE(id, pred)                                                                                     \
  do {                                                                                                                \
    const unsigned long long act_ = __ballot(true), m_ = __ballot(pred);                                              \
    if (m_ && (int)(threadIdx.x & 63) == __ffsll((long long)act_) - 1) {                                              \
      atomicAdd(&lane_words()[2 * (id)], 64u);                                                                        \
      atomicAdd(&lane_words()[2 * (id) + 1], (uint32_t)__popcll(m_));                                                 \
      atomicAdd(&lane_words()[2 * kLaneLoops + 4 * (id) + lane_role()], 1u);                                          \
    }                                                                                                                 \
  } while (0)
// (kernel: 0 set-up, 1 tile.  The first lane of every wave reads where it runs from the hardware-id register -- id 4: SIMD in
// bits 5:4, CU / shader array / shader engine in bits 15:8; id 20: the XCD -- and counts the wave in two 4 x 4 tables, wave
// index against SIMD: one over the whole chip, one for the waves of a single CU, the one that the batch's first wave ran on.
// A table that is even over the chip could still hide CUs that each keep a placement of their own.)
#define RTUF_LANES_INIT(kernel)                                                                                       \
  do {                                                                                                                \
    for (int i_ = threadIdx.x; i_ < 6 * kLaneLoops; i_ += blockDim.x) lane_words()[i_] = 0u;                          \
    __syncthreads();                                                                                                  \
    if ((threadIdx.x & 63u) == 0u) {                                                                                  \
      const uint32_t simd_ = __builtin_amdgcn_s_getreg(4 | (4 << 6) | (1 << 11)), w_ = (threadIdx.x >> 6) & 3u;       \
      const uint32_t cu_ = 1u + (__builtin_amdgcn_s_getreg(4 | (8 << 6) | (7 << 11)) | (__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) << 8)); \
      unsigned long long* t_ = a.counters->shard[0].lane_roles + 4 * kLaneLoops + (kernel) * kRoleTables * 16;        \
      atomicAdd(&t_[w_ * 4 + simd_], 1ull);                                                                           \
      unsigned long long* key_ = a.counters->shard[0].lane_roles + kLaneRoleWords - 2 + (kernel);                     \
      const unsigned long long was_ = atomicCAS(key_, 0ull, (unsigned long long)cu_);                                 \
      if (was_ == 0ull || was_ == (unsigned long long)cu_) atomicAdd(&t_[16 + w_ * 4 + simd_], 1ull);                 \
    }                                                                                                                 \
  } while (0)
#define RTUF_LANES_FLUSH(shard)                                                                                       \
  do {                                                                                                                \
    __syncthreads();                                                                                                  \
    if ((int)threadIdx.x < kLaneLoops && (lane_words()[2 * threadIdx.x] | lane_words()[2 * threadIdx.x + 1])) {        \
      atomicAdd(&(shard).lane_slots[threadIdx.x], (unsigned long long)lane_words()[2 * threadIdx.x]);                 \
      atomicAdd(&(shard).lane_live[threadIdx.x], (unsigned long long)lane_words()[2 * threadIdx.x + 1]);              \
    }                                                                                                                 \
    if ((int)threadIdx.x < 4 * kLaneLoops && lane_words()[2 * kLaneLoops + threadIdx.x])                              \
      atomicAdd(&(shard).lane_roles[threadIdx.x], (unsigned long long)lane_words()[2 * kLaneLoops + threadIdx.x]);    \
  } while (0)
#else
#define RTUF_LANES(id, pred) ((void)0)
#define RTUF_LANES_LIVE(id, pred) ((void)0)
#define RTUF_LANES_INIT(kernel) ((void)0)
#define RTUF_LANES_FLUSH(shard) ((void)0)
#endif

// ---------------------------------------------------------------------------------------
// float32 matrix stack (GL semantics: every glMultMatrixd rounds its argument to float and
// multiplies in float32, products accumulated left to right, no fused multiply-add)
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void matmul4(float* __restrict__ out, const float* a, const float* b)
{
  float p[16];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float ai0 = a[i], ai1 = a[4 + i], ai2 = a[8 + i], ai3 = a[12 + i];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float s = __fmul_rn(ai0, b[4 * j]);
      s = __fadd_rn(s, __fmul_rn(ai1, b[4 * j + 1]));
      s = __fadd_rn(s, __fmul_rn(ai2, b[4 * j + 2]));
      s = __fadd_rn(s, __fmul_rn(ai3, b[4 * j + 3]));
      p[4 * j + i] = s;
    }
  }
#pragma unroll
  for (int k = 0; k < 16; k++) out[k] = p[k];
}

__device__ __forceinline__ void mult_d(float* top, const double* m)
{
  float f[16];
#pragma unroll
  for (int k = 0; k < 16; k++) f[k] = (float)m[k];
  matmul4(top, top, f);
}

__device__ __forceinline__ void vs_position(const float* __restrict__ M, float x, float y, float z, float* c)
{
#pragma unroll
  for (int r = 0; r < 4; r++) {
    float s = __fmul_rn(M[r], x);
    s = __fadd_rn(s, __fmul_rn(M[4 + r], y));
    s = __fadd_rn(s, __fmul_rn(M[8 + r], z));
    s = __fadd_rn(s, M[12 + r]);
    c[r] = s;
  }
}

__device__ __forceinline__ unsigned clipmask_of(const float* c)
{
  unsigned m = 0;
  if (c[0] > c[3]) m |= 1u;
  if (0.0f > __fadd_rn(c[0], c[3])) m |= 2u;
  if (c[1] > c[3]) m |= 4u;
  if (0.0f > __fadd_rn(c[1], c[3])) m |= 8u;
  if (0.0f > __fadd_rn(c[2], c[3])) m |= 16u;
  if (c[2] > c[3]) m |= 32u;
  return m;
}

struct Win { float x, y, z; };

// viewport transform of a shaded vertex (fused multiply-add form)
__device__ __forceinline__ Win viewport_vs(const float* c, float sx, float sy)
{
  const float rhw = __fdiv_rn(1.0f, c[3]);
  Win w;
  w.x = __fmaf_rn(__fmul_rn(c[0], rhw), sx, sx);
  w.y = __fmaf_rn(__fmul_rn(c[1], rhw), sy, sy);
  w.z = __fmaf_rn(__fmul_rn(c[2], rhw), 0.5f, 0.5f);
  return w;
}

// viewport transform of a vertex made by the clipper (separate multiply and add)
__device__ __forceinline__ Win viewport_clip(const float* c, float sx, float sy)
{
  const float oow = __fdiv_rn(1.0f, c[3]);
  Win w;
  w.x = __fadd_rn(__fmul_rn(__fmul_rn(c[0], oow), sx), sx);
  w.y = __fadd_rn(__fmul_rn(__fmul_rn(c[1], oow), sy), sy);
  w.z = __fadd_rn(__fmul_rn(__fmul_rn(c[2], oow), 0.5f), 0.5f);
  return w;
}

// ---------------------------------------------------------------------------------------
// pose_kernel: one thread per (stream, draw).  Draw index == n_draws is the background quad.
// ---------------------------------------------------------------------------------------

__global__ void pose_kernel(PoseArgs a)
{
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int per = a.n_draws + 1;
  // first kernel of a batch that every configuration runs: it also zeroes the batch's counters
  // (statistics, clip lists, work-list length), which saves a separate fill launch per batch
  // (one block of counters per launch group of the batch)
  for (int cb = blockIdx.x; cb < a.n_counters; cb += gridDim.x) {
    uint32_t* w = reinterpret_cast<uint32_t*>(a.counters + cb);
    for (int i = threadIdx.x; i < (int)(sizeof(Counters) / 4); i += blockDim.x) w[i] = 0u;
  }
  // ... and says so in the batch slot's status word: this many launch groups have not finished (see kStatus* in rtuf_device.h)
  if (gid == 0) *a.status = (uint32_t)a.n_counters;
  if (gid >= a.n_streams * per) return;
  const int s = gid / per, d = gid - s * per;
  const Camera& cam = a.cams[s];

  float proj[16], mv[16];
#pragma unroll
  for (int k = 0; k < 16; k++) proj[k] = mv[k] = (k % 5 == 0) ? 1.0f : 0.0f;
  mult_d(proj, cam.projection);
  {
    // gluLookAt(0,0,0, 0,0,1, 0,1,0) == diag(-1,1,-1,1), then glTranslated(-0,-0,-0)
    const float la[16] = {-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1};
    matmul4(mv, mv, la);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      float t = __fmul_rn(mv[r], -0.0f);
      t = __fadd_rn(t, __fmul_rn(mv[4 + r], -0.0f));
      t = __fadd_rn(t, __fmul_rn(mv[8 + r], -0.0f));
      mv[12 + r] = __fadd_rn(t, mv[12 + r]);
    }
  }
  float* out = a.mvp + ((size_t)s * per + d) * 16;
  if (d == a.n_draws) {
    // background quad (urdf_filter.cpp:591-596): drawn before the camera transforms
    float m[16];
    matmul4(m, proj, mv);
#pragma unroll
    for (int k = 0; k < 16; k++) out[k] = m[k];
    const float zq = (float)((double)a.z_far * 0.99);
    const float qx[4] = {-100.0f, 100.0f, 100.0f, -100.0f};
    const float qy[4] = {-100.0f, -100.0f, 100.0f, 100.0f};
    float c0[4];
    bool constant = true, covers = true;
    unsigned andm = ~0u;
    for (int i = 0; i < 4; i++) {
      float c[4];
      vs_position(m, qx[i], qy[i], zq, c);
      if (i == 0) { c0[0] = c[0]; c0[1] = c[1]; c0[2] = c[2]; c0[3] = c[3]; }
      if (c[2] != c0[2] || c[3] != c0[3]) constant = false;
      const unsigned cm = clipmask_of(c);
      if (cm & 48u) constant = false;               // must lie strictly inside near/far
      if (!(c[3] > 0.0f)) constant = false;
      // corner i must be outside the frustum sideways by a wide margin in both x and y
      if (!(fabsf(c[0]) > 2.0f * c[3] && fabsf(c[1]) > 2.0f * c[3])) covers = false;
      andm &= cm;
    }
    // the four corners must lie in four different xy quadrants (quad surrounds the frustum axis)
    float cA[4], cB[4], cC[4];
    vs_position(m, qx[1], qy[1], zq, cA);
    vs_position(m, qx[2], qy[2], zq, cB);
    vs_position(m, qx[3], qy[3], zq, cC);
    const bool quadrants = (c0[0] < 0) != (cA[0] < 0) && (cA[1] < 0) != (cB[1] < 0) &&
                           (cB[0] < 0) != (cC[0] < 0) && (cC[1] < 0) != (c0[1] < 0);
    const bool ok = constant && covers && quadrants && andm == 0;
    // constant plane: every clipped vertex keeps z_clip and w, so its window z is (z/w)*0.5+0.5
    const float zw = __fadd_rn(__fmul_rn(__fmul_rn(c0[2], __fdiv_rn(1.0f, c0[3])), 0.5f), 0.5f);
    BgInfo bi;
    bi.z = zw;
    bi.mode = ok ? 1u : 0u;
    bi.thr = __fsub_rn(__fdiv_rn(a.sc_num, __fsub_rn(zw, a.sc_off)), a.max_diff);                  // shade_threshold(zw)
    bi.z24 = z24_of(zw);
    a.bg[s] = bi;
    return;
  }
  const Draw dr = a.draws[d];
  mult_d(mv, cam.offset_inv);
  mult_d(mv, cam.cam_tf);
  mult_d(mv, a.link_tf + ((size_t)s * a.n_links + dr.link) * 16);
  if (dr.pre_op == 1) {            // glScalef
#pragma unroll
    for (int r = 0; r < 4; r++) {
      mv[r] = __fmul_rn(mv[r], dr.op[0]);
      mv[4 + r] = __fmul_rn(mv[4 + r], dr.op[1]);
      mv[8 + r] = __fmul_rn(mv[8 + r], dr.op[2]);
    }
  } else if (dr.pre_op == 2) {     // glTranslatef
#pragma unroll
    for (int r = 0; r < 4; r++) {
      float t = __fmul_rn(mv[r], dr.op[0]);
      t = __fadd_rn(t, __fmul_rn(mv[4 + r], dr.op[1]));
      t = __fadd_rn(t, __fmul_rn(mv[8 + r], dr.op[2]));
      mv[12 + r] = __fadd_rn(t, mv[12 + r]);
    }
  }
  float m[16];
  matmul4(m, proj, mv);
#pragma unroll
  for (int k = 0; k < 16; k++) out[k] = m[k];
}

// ---------------------------------------------------------------------------------------
// fk_kernel: forward kinematics in double precision, one thread per (stream, frame).  The chain
// root -> frame is multiplied top-down, T_child = (T_parent * origin) * motion(q), the same
// association order as the host-side forward kinematics.
// ---------------------------------------------------------------------------------------
struct Tf12 { double m[9]; double o[3]; };

__device__ __forceinline__ Tf12 tf_mul(const Tf12& a, const Tf12& b)
{
  Tf12 r;
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++)
      r.m[3 * i + j] = __dadd_rn(__dadd_rn(__dmul_rn(a.m[3 * i], b.m[j]), __dmul_rn(a.m[3 * i + 1], b.m[3 + j])), __dmul_rn(a.m[3 * i + 2], b.m[6 + j]));
    r.o[i] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(a.m[3 * i], b.o[0]), __dmul_rn(a.m[3 * i + 1], b.o[1])), __dmul_rn(a.m[3 * i + 2], b.o[2])), a.o[i]);
  }
  return r;
}

__device__ __forceinline__ Tf12 tf_load(const double* p)
{
  Tf12 t;
#pragma unroll
  for (int k = 0; k < 9; k++) t.m[k] = p[k];
  t.o[0] = p[9]; t.o[1] = p[10]; t.o[2] = p[11];
  return t;
}

__device__ __forceinline__ Tf12 tf_from_quat(double x, double y, double z, double w)
{
  // Matrix3x3::setRotation
  Tf12 t;
  const double d = x * x + y * y + z * z + w * w;
  const double s = 2.0 / d;
  const double xs = x * s, ys = y * s, zs = z * s;
  const double wx = w * xs, wy = w * ys, wz = w * zs;
  const double xx = x * xs, xy = x * ys, xz = x * zs;
  const double yy = y * ys, yz = y * zs, zz = z * zs;
  t.m[0] = 1.0 - (yy + zz); t.m[1] = xy - wz; t.m[2] = xz + wy;
  t.m[3] = xy + wz; t.m[4] = 1.0 - (xx + zz); t.m[5] = yz - wx;
  t.m[6] = xz - wy; t.m[7] = yz + wx; t.m[8] = 1.0 - (xx + yy);
  t.o[0] = t.o[1] = t.o[2] = 0.0;
  return t;
}

__device__ __forceinline__ void tf_store_gl(const Tf12& t, double* g)
{
  g[0] = t.m[0]; g[1] = t.m[3]; g[2] = t.m[6]; g[3] = 0.0;
  g[4] = t.m[1]; g[5] = t.m[4]; g[6] = t.m[7]; g[7] = 0.0;
  g[8] = t.m[2]; g[9] = t.m[5]; g[10] = t.m[8]; g[11] = 0.0;
  g[12] = t.o[0]; g[13] = t.o[1]; g[14] = t.o[2]; g[15] = 1.0;
}

// src/urdf_filter.cpp:607-611: the camera origin moves by camera_tx_ along the camera transform's x axis
// ("right" = rotation * (1,0,0)), then by camera_ty_ along its y axis ("down")
__device__ __forceinline__ void apply_camera_shift(Tf12& t, const double* shift)
{
  const double tx = shift[0], ty = shift[1];
#pragma unroll
  for (int i = 0; i < 3; i++) t.o[i] = __dadd_rn(t.o[i], __dmul_rn(t.m[3 * i], tx));
#pragma unroll
  for (int i = 0; i < 3; i++) t.o[i] = __dadd_rn(t.o[i], __dmul_rn(t.m[3 * i + 1], ty));
}

__device__ Tf12 fk_frame(const FkArgs& a, int s, int frame)
{
  int chain[64];
  int n = 0;
  for (int f = frame; f >= 0 && n < 64; f = a.parent[f]) chain[n++] = f;
  Tf12 t;
  if (a.root_tf) t = tf_load(a.root_tf + (size_t)s * 12);
  else { for (int k = 0; k < 9; k++) t.m[k] = (k % 4 == 0) ? 1.0 : 0.0; t.o[0] = t.o[1] = t.o[2] = 0.0; }
  for (int k = n - 1; k >= 0; k--) {
    const int f = chain[k];
    if (a.parent[f] < 0) continue;                  // the root frame carries no joint
    t = tf_mul(t, tf_load(a.joint_origin + (size_t)f * 12));
    const int jt = a.joint_type[f];
    if (jt == 1) {
      const double q = a.q[(size_t)s * a.n_frames + f];
      const double ax = a.joint_axis[3 * f], ay = a.joint_axis[3 * f + 1], az = a.joint_axis[3 * f + 2];
      const double nn = sqrt(ax * ax + ay * ay + az * az);
      const double ux = nn > 0 ? ax / nn : 1.0, uy = nn > 0 ? ay / nn : 0.0, uz = nn > 0 ? az / nn : 0.0;
      const double sh = sin(0.5 * q), ch = cos(0.5 * q);
      t = tf_mul(t, tf_from_quat(ux * sh, uy * sh, uz * sh, ch));
    } else if (jt == 2) {
      const double q = a.q[(size_t)s * a.n_frames + f];
      Tf12 m;
      for (int k2 = 0; k2 < 9; k2++) m.m[k2] = (k2 % 4 == 0) ? 1.0 : 0.0;
      m.o[0] = a.joint_axis[3 * f] * q; m.o[1] = a.joint_axis[3 * f + 1] * q; m.o[2] = a.joint_axis[3 * f + 2] * q;
      t = tf_mul(t, m);
    }
  }
  return t;
}

__global__ void fk_kernel(FkArgs a)
{
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int per = a.n_links_model + 1;
  if (gid >= a.n_streams * per) return;
  const int s = gid / per, l = gid - s * per;
  if (!a.enabled[s]) return;
  if (l < a.n_links_model) {
    // link matrix = (fixed<-frame) * link_offset   (Renderable::applyTransform)
    const Tf12 t = tf_mul(fk_frame(a, s, a.link_frame[l]), tf_load(a.link_offset + (size_t)l * 12));
    tf_store_gl(t, a.link_tf + ((size_t)s * a.n_links_total + a.link_base + l) * 16);
  } else if (a.camera_frame >= 0) {
    // camera_transform = lookupTransform(cam_frame, fixed_frame) = inverse(fixed<-camera)
    const Tf12 t = fk_frame(a, s, a.camera_frame);
    Tf12 inv;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) inv.m[3 * i + j] = t.m[3 * j + i];
    for (int i = 0; i < 3; i++) inv.o[i] = inv.m[3 * i] * (-t.o[0]) + inv.m[3 * i + 1] * (-t.o[1]) + inv.m[3 * i + 2] * (-t.o[2]);
    apply_camera_shift(inv, a.cams[s].shift);
    tf_store_gl(inv, a.cams[s].cam_tf);
  }
}

// Same arithmetic, organised as a tree sweep: one workgroup per stream keeps every frame's
// fixed<-frame transform in LDS and fills it level by level (all frames of one depth in parallel,
// T_child = (T_parent * origin) * motion(q)), then the links and the camera read it.  Used when the
// tree fits in LDS (kFkMaxFrames frames); fk_kernel above is the general fallback.
constexpr int kFkMaxFrames = 256;
__global__ __launch_bounds__(kFkMaxFrames) void fk_tree_kernel(FkArgs a)
{
  __shared__ double s_t[kFkMaxFrames][12];
  const int s = blockIdx.x;
  if (!a.enabled[s]) return;
  const int f = threadIdx.x;                 // one frame per lane; everything it needs is fetched up front
  const bool have = f < a.n_frames;
  int parent = -1, depth = -1;
  Tf12 origin, motion;
  bool has_motion = false;
  if (have) {
    parent = a.parent[f];
    depth = a.depth[f];
    if (depth > 0) {
      origin = tf_load(a.joint_origin + (size_t)f * 12);
      const int jt = a.joint_type[f];
      if (jt == 1) {
        const double q = a.q[(size_t)s * a.n_frames + f];
        const double ax = a.joint_axis[3 * f], ay = a.joint_axis[3 * f + 1], az = a.joint_axis[3 * f + 2];
        const double nn = sqrt(ax * ax + ay * ay + az * az);
        const double ux = nn > 0 ? ax / nn : 1.0, uy = nn > 0 ? ay / nn : 0.0, uz = nn > 0 ? az / nn : 0.0;
        const double sh = sin(0.5 * q), ch = cos(0.5 * q);
        motion = tf_from_quat(ux * sh, uy * sh, uz * sh, ch);
        has_motion = true;
      } else if (jt == 2) {
        const double q = a.q[(size_t)s * a.n_frames + f];
        for (int k2 = 0; k2 < 9; k2++) motion.m[k2] = (k2 % 4 == 0) ? 1.0 : 0.0;
        motion.o[0] = a.joint_axis[3 * f] * q; motion.o[1] = a.joint_axis[3 * f + 1] * q; motion.o[2] = a.joint_axis[3 * f + 2] * q;
        has_motion = true;
      }
    }
  }
  for (int d = 0; d <= a.max_depth; d++) {
    if (have && depth == d) {
      Tf12 t;
      if (d == 0) {
        if (a.root_tf) t = tf_load(a.root_tf + (size_t)s * 12);
        else { for (int k = 0; k < 9; k++) t.m[k] = (k % 4 == 0) ? 1.0 : 0.0; t.o[0] = t.o[1] = t.o[2] = 0.0; }
      } else {
        t = tf_mul(tf_load(s_t[parent]), origin);
        if (has_motion) t = tf_mul(t, motion);
      }
#pragma unroll
      for (int k = 0; k < 9; k++) s_t[f][k] = t.m[k];
      s_t[f][9] = t.o[0]; s_t[f][10] = t.o[1]; s_t[f][11] = t.o[2];
    }
    __syncthreads();
  }
  for (int l = threadIdx.x; l < a.n_links_model; l += blockDim.x) {
    const Tf12 t = tf_mul(tf_load(s_t[a.link_frame[l]]), tf_load(a.link_offset + (size_t)l * 12));
    tf_store_gl(t, a.link_tf + ((size_t)s * a.n_links_total + a.link_base + l) * 16);
  }
  if (threadIdx.x == 0 && a.camera_frame >= 0) {
    const Tf12 t = tf_load(s_t[a.camera_frame]);
    Tf12 inv;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) inv.m[3 * i + j] = t.m[3 * j + i];
    for (int i = 0; i < 3; i++) inv.o[i] = inv.m[3 * i] * (-t.o[0]) + inv.m[3 * i + 1] * (-t.o[1]) + inv.m[3 * i + 2] * (-t.o[2]);
    apply_camera_shift(inv, a.cams[s].shift);
    tf_store_gl(inv, a.cams[s].cam_tf);
  }
}

// ---------------------------------------------------------------------------------------
// triangle set-up
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ int snap(float v)
{
  return __float2int_rn(__fmul_rn(__fsub_rn(v, 0.5f), 256.0f));
}

// Integer edge functions + bounding box of an ORIENTED (area > 0) snapped triangle.  Used by the
// set-up kernel (fragment path) and by the tile kernel when it unpacks a 32-byte bin record.
__device__ __forceinline__ void edges_from_snapped(int x0, int y0, int x1, int y1, int x2, int y2, int width, int height,
                                                   TriRec& r)
{
  const int minx = min(x0, min(x1, x2)), maxx = max(x0, max(x1, x2));
  const int miny = min(y0, min(y1, y2)), maxy = max(y0, max(y1, y2));
  const int bx0 = max((minx + 255) >> 8, 0), bx1 = min((maxx - 1) >> 8, width - 1);
  const int by0 = max((miny + 255) >> 8, 0), by1 = min((maxy - 1) >> 8, height - 1);
  const int xs[3] = {x0, x1, x2}, ys[3] = {y0, y1, y2};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const int j = (i + 1) % 3;
    const int dcdx = ys[i] - ys[j];
    const int dcdy = xs[i] - xs[j];
    r.A[i] = -dcdx;
    r.B[i] = dcdy;
    r.C[i] = edge_constant(dcdx, dcdy, xs[i], ys[i]);
  }
  r.bbx = (uint32_t)bx0 | ((uint32_t)bx1 << 16);
  r.bby = (uint32_t)by0 | ((uint32_t)by1 << 16);
}

__device__ __forceinline__ int sext21(int v) { return (v << 11) >> 11; }

// Snap, sub-pixel cull, orientation.  Returns false when the triangle covers no pixel centre or is
// degenerate; on success the snapped coordinates are oriented (area > 0, v0/v1 swapped if needed)
// and bx/by hold the inclusive pixel bounding box.
__device__ __forceinline__ bool orient_and_bound(Win& v0, Win& v1, const Win& v2, int width, int height,
                                                 int& x0, int& y0, int& x1, int& y1, int& x2, int& y2,
                                                 int& bx0, int& bx1, int& by0, int& by1)
{
  // vertices of unclipped triangles lie inside the frustum: snapped values are in [-128, 2048*256+128]
  // (clipper-made vertices, a few units more, never come here).
  // The (value-preserving) 21-bit sign extension tells the compiler so, which turns the 64-bit
  // products below into full-rate 24-bit multiplies.
  // x0..y2 come in as the snapped coordinates of phase 1 (s_snap): snap(v.x), snap(v.y)
  x0 = sext21(x0); y0 = sext21(y0);
  x1 = sext21(x1); y1 = sext21(y1);
  x2 = sext21(x2); y2 = sext21(y2);
  const int minx = min(x0, min(x1, x2)), maxx = max(x0, max(x1, x2));
  const int miny = min(y0, min(y1, y2)), maxy = max(y0, max(y1, y2));
  bx0 = max((minx + 255) >> 8, 0); bx1 = min((maxx - 1) >> 8, width - 1);
  by0 = max((miny + 255) >> 8, 0); by1 = min((maxy - 1) >> 8, height - 1);
  if (bx1 < bx0 || by1 < by0) return false;
  const long long area = (long long)(x0 - x1) * (y2 - y0) - (long long)(x2 - x0) * (y0 - y1);
  if (area == 0) return false;
  if (area < 0) {   // orient: swap vertices 0 and 1 (fixed and float)
    int t = x0; x0 = x1; x1 = t;
    t = y0; y0 = y1; y1 = t;
    Win tw = v0; v0 = v1; v1 = tw;
  }
  return true;
}

// z plane from the unsnapped float vertices (lp_state_setup.c order)
__device__ __forceinline__ void z_plane(const Win& v0, const Win& v1, const Win& v2, float& a0, float& dzdx, float& dzdy)
{
  const float x0c = __fsub_rn(v0.x, 0.5f), y0c = __fsub_rn(v0.y, 0.5f);
  const float dx01 = __fsub_rn(v0.x, v1.x), dy01 = __fsub_rn(v0.y, v1.y);
  const float dx20 = __fsub_rn(v2.x, v0.x), dy20 = __fsub_rn(v2.y, v0.y);
  const float ooa = __fdiv_rn(1.0f, __fsub_rn(__fmul_rn(dx01, dy20), __fmul_rn(dy01, dx20)));
  const float dy20o = __fmul_rn(dy20, ooa), dy01o = __fmul_rn(dy01, ooa);
  const float dx20o = __fmul_rn(dx20, ooa), dx01o = __fmul_rn(dx01, ooa);
  const float da01 = __fsub_rn(v0.z, v1.z), da20 = __fsub_rn(v2.z, v0.z);
  dzdx = __fsub_rn(__fmul_rn(da01, dy20o), __fmul_rn(da20, dy01o));
  dzdy = __fsub_rn(__fmul_rn(da20, dx01o), __fmul_rn(da01, dx20o));
  a0 = __fsub_rn(v0.z, __fadd_rn(__fmul_rn(dzdx, x0c), __fmul_rn(dzdy, y0c)));
}

// Smallest / largest value the z plane takes over an inclusive rectangle of pixel coordinates, evaluated exactly like
// fragment() does: fma(dzdy, y, fma(dzdx, x, a0)) is monotonic in x and in y (rounding is monotonic), so the extreme is at
// the corner the two slopes point away from / towards.  NaN when the plane is not finite there: callers treat NaN as
// "unknown" (z24_of(NaN) = 0 never drops anything; a NaN maximum publishes no bound).
__device__ __forceinline__ float plane_min(float a0, float dzdx, float dzdy, int x0, int x1, int y0, int y1)
{
  const float xm = (float)(dzdx < 0.0f ? x1 : x0), ym = (float)(dzdy < 0.0f ? y1 : y0);
  return __fmaf_rn(dzdy, ym, __fmaf_rn(dzdx, xm, a0));
}
__device__ __forceinline__ float plane_max(float a0, float dzdx, float dzdy, int x0, int x1, int y0, int y1)
{
  const float xm = (float)(dzdx < 0.0f ? x0 : x1), ym = (float)(dzdy < 0.0f ? y0 : y1);
  return __fmaf_rn(dzdy, ym, __fmaf_rn(dzdx, xm, a0));
}
// A record is "near" when its plane may reach window z <= 0.5 somewhere in its bounding box (the same margin as the
// fragment path's hand-over: 0.51; a NaN counts as near).  Only near records take part in the tile kernel's exact-z pass.
__device__ __forceinline__ uint32_t near_bit(float a0, float dzdx, float dzdy, int bx0, int bx1, int by0, int by1)
{
  return !(plane_min(a0, dzdx, dzdy, bx0, bx1, by0, by1) >= 0.51f) ? kNearBit : 0u;
}

__device__ __forceinline__ PackedTri pack_record(int x0, int y0, int x1, int y1, int x2, int y2, float a0, float dzdx,
                                                 float dzdy, uint32_t order)
{
  // snapped coordinates of in-frustum vertices lie in [-128, 2048*256 + 128]; vertices made by the clipper can be a
  // few 1/256 px outside that (their interpolation is rounded): 20 bits after the bias of kCoordBias
  PackedTri pk;
  pk.v01 = (unsigned long long)(uint32_t)(x0 + kCoordBias) | ((unsigned long long)(uint32_t)(y0 + kCoordBias) << 20) | ((unsigned long long)(uint32_t)(x1 + kCoordBias) << 40);
  pk.v12 = (unsigned long long)(uint32_t)(y1 + kCoordBias) | ((unsigned long long)(uint32_t)(x2 + kCoordBias) << 20) | ((unsigned long long)(uint32_t)(y2 + kCoordBias) << 40);
  pk.a0 = a0; pk.dzdx = dzdx; pk.dzdy = dzdy; pk.order = order;
  return pk;
}

// Builds the raster record of one window-space triangle.  Returns false when it covers no
// pixel centre of the width x height frame.  `pk` receives the 32-byte bin form.
__device__ __forceinline__ bool make_record(Win v0, Win v1, Win v2, uint32_t order, int width, int height,
                                            TriRec& r, PackedTri& pk)
{
  int x0 = snap(v0.x), y0 = snap(v0.y);
  int x1 = snap(v1.x), y1 = snap(v1.y);
  const int x2 = snap(v2.x), y2 = snap(v2.y);
  // bounding box of covered pixel centres first: most mesh triangles are sub-pixel and end here
  const int minx = min(x0, min(x1, x2)), maxx = max(x0, max(x1, x2));
  const int miny = min(y0, min(y1, y2)), maxy = max(y0, max(y1, y2));
  int bx0 = (minx + 255) >> 8, bx1 = (maxx - 1) >> 8;
  int by0 = (miny + 255) >> 8, by1 = (maxy - 1) >> 8;
  bx0 = max(bx0, 0); by0 = max(by0, 0);
  bx1 = min(bx1, width - 1); by1 = min(by1, height - 1);
  if (bx1 < bx0 || by1 < by0) return false;
  const long long area = (long long)(x0 - x1) * (y2 - y0) - (long long)(x2 - x0) * (y0 - y1);
  if (area == 0) return false;
  if (area < 0) {   // orient: swap vertices 0 and 1 (fixed and float)
    int t = x0; x0 = x1; x1 = t;
    t = y0; y0 = y1; y1 = t;
    Win tw = v0; v0 = v1; v1 = tw;
  }
  edges_from_snapped(x0, y0, x1, y1, x2, y2, width, height, r);
  // z plane from the unsnapped float vertices
  const float x0c = __fsub_rn(v0.x, 0.5f), y0c = __fsub_rn(v0.y, 0.5f);
  const float dx01 = __fsub_rn(v0.x, v1.x), dy01 = __fsub_rn(v0.y, v1.y);
  const float dx20 = __fsub_rn(v2.x, v0.x), dy20 = __fsub_rn(v2.y, v0.y);
  const float ooa = __fdiv_rn(1.0f, __fsub_rn(__fmul_rn(dx01, dy20), __fmul_rn(dy01, dx20)));
  const float dy20o = __fmul_rn(dy20, ooa), dy01o = __fmul_rn(dy01, ooa);
  const float dx20o = __fmul_rn(dx20, ooa), dx01o = __fmul_rn(dx01, ooa);
  const float da01 = __fsub_rn(v0.z, v1.z), da20 = __fsub_rn(v2.z, v0.z);
  r.dzdx = __fsub_rn(__fmul_rn(da01, dy20o), __fmul_rn(da20, dy01o));
  r.dzdy = __fsub_rn(__fmul_rn(da20, dx01o), __fmul_rn(da01, dx20o));
  r.a0 = __fsub_rn(v0.z, __fadd_rn(__fmul_rn(r.dzdx, x0c), __fmul_rn(r.dzdy, y0c)));
  r.order = order;
  r.pad = 0;
  // snapped coordinates of in-frustum vertices lie in [-128, 2048*256 + 128]; vertices made by the clipper can be a
  // few 1/256 px outside that (their interpolation is rounded): 20 bits after the bias of kCoordBias
  pk.v01 = (unsigned long long)(uint32_t)(x0 + kCoordBias) | ((unsigned long long)(uint32_t)(y0 + kCoordBias) << 20) | ((unsigned long long)(uint32_t)(x1 + kCoordBias) << 40);
  pk.v12 = (unsigned long long)(uint32_t)(y1 + kCoordBias) | ((unsigned long long)(uint32_t)(x2 + kCoordBias) << 20) | ((unsigned long long)(uint32_t)(y2 + kCoordBias) << 40);
  pk.a0 = r.a0; pk.dzdx = r.dzdx; pk.dzdy = r.dzdy;
  pk.order = order | near_bit(r.a0, r.dzdx, r.dzdy, (int)(r.bbx & 0xffff), (int)(r.bbx >> 16), (int)(r.bby & 0xffff), (int)(r.bby >> 16));
  return true;
}

__device__ __forceinline__ TriRec unpack_record(const PackedTri& pk, int width, int height)
{
  TriRec r;
  const int x0 = (int)(pk.v01 & 0xfffffu) - kCoordBias, y0 = (int)((pk.v01 >> 20) & 0xfffffu) - kCoordBias, x1 = (int)((pk.v01 >> 40) & 0xfffffu) - kCoordBias;
  const int y1 = (int)(pk.v12 & 0xfffffu) - kCoordBias, x2 = (int)((pk.v12 >> 20) & 0xfffffu) - kCoordBias, y2 = (int)((pk.v12 >> 40) & 0xfffffu) - kCoordBias;
  edges_from_snapped(x0, y0, x1, y1, x2, y2, width, height, r);
  r.a0 = pk.a0; r.dzdx = pk.dzdx; r.dzdy = pk.dzdy; r.order = pk.order & kOrderMask; r.pad = pk.order >> 31;
  return r;
}

__device__ __forceinline__ void store_record(PackedTri* dst, const PackedTri& r)
{
  const uint4* s = reinterpret_cast<const uint4*>(&r);
  uint4* d = reinterpret_cast<uint4*>(dst);
  d[0] = s[0]; d[1] = s[1];
}

// Records whose bounding box touches more than kCoopTiles tiles (the robot's own arm in front of the camera, clipped
// near-plane triangles, walls) are not appended to their bins here: they go on the shard's big-record list (one
// reservation per wave), and bigrec_kernel appends every list entry with a wave of its own.  Appending them where they
// are made costs a wave one atomic round trip per record, and such records come in runs (a wall's fan: hundreds of
// (record, tile) pairs in a handful of waves while the rest of the GPU has finished).
constexpr int kCoopTiles = 4;            // (8: the same; 2: +20 us of bigrec_kernel; 1: every straddling record on the lists, 0.5 ms)
#ifndef RTUF_FRONT_AREA
#define RTUF_FRONT_AREA 24
#endif
constexpr int kFrontArea = RTUF_FRONT_AREA;      // boxes up to this many pixel centres are binned from the front of a bin
__device__ __forceinline__ void list_big_records_wave(const SetupArgs& a, int shard_id, int slot, bool big, const PackedTri& pk)
{
  const int lane = threadIdx.x & 63;
  const unsigned long long bm = __ballot(big);
  const int leader = __ffsll((long long)bm) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(&a.counters->shard[shard_id].big_count, (uint32_t)__popcll(bm));
  base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
  if (big) {
    const uint32_t idx = base + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull));
    if (idx < a.big_capacity) {          // (an over-full list is detected from the counter and the batch run again)
      uint4* dst = reinterpret_cast<uint4*>(a.big_list + (size_t)shard_id * a.big_capacity + idx);
      const uint4* src = reinterpret_cast<const uint4*>(&pk);
      dst[0] = src[0]; dst[1] = src[1]; dst[2] = make_uint4((uint32_t)slot, 0u, 0u, 0u);
    }
  }
}

// Wave-cooperative form: all 64 lanes call it; lanes with `have` own a record.  Lanes that
// target the same bin are grouped with ballots (ALU only), then every group leader issues its
// atomicAdd in the SAME instruction, so a wave pays one atomic round trip per tile index
// instead of one per distinct bin; group members get consecutive slots, which makes the
// 32-byte record stores of neighbouring mesh triangles contiguous.
__device__ __forceinline__ uint32_t emit_record_wave(const SetupArgs& a, int shard_id, int slot, bool have, uint32_t bbx, uint32_t bby, const PackedTri& pk)
{
  const int lane = threadIdx.x & 63;
  int tx0 = 0, tx1 = -1, ty0 = 0, ty1 = -1;
  if (have) {
    tx0 = (int)(bbx & 0xffff) / kTileW; tx1 = (int)(bbx >> 16) / kTileW;
    ty0 = (int)(bby & 0xffff) / kTileH; ty1 = (int)(bby >> 16) / kTileH;
  }
  const int tiles = a.tiles_x * a.tiles_y;
  uint32_t n = 0;
  // Two size classes per bin: records with a box of at most kFrontArea pixel centres fill the bin from
  // the front, larger ones from the back, so the tile kernel's waves get boxes of similar size (its
  // lane-per-triangle walk runs as long as the largest box in the wave).
  const int cls = ((int)(bbx >> 16) - (int)(bbx & 0xffff) + 1) * ((int)(bby >> 16) - (int)(bby & 0xffff) + 1) > kFrontArea ? 1 : 0;
  const bool big = have && (tx1 - tx0 + 1) * (ty1 - ty0 + 1) > kCoopTiles;
  if (__ballot(big)) list_big_records_wave(a, shard_id, slot, big, pk);          // (their bin entries are counted by bigrec_kernel)
  have = have && !big;
  int tx = tx0, ty = ty0;                  // walks the touched tiles row by row
  for (;;) {
    const bool act = have && ty <= ty1;
    unsigned long long pending = __ballot(act);
    if (!pending) break;
    const int bin = act ? 2 * (__mul24(slot, tiles) + __mul24(ty, a.tiles_x) + tx) + cls : -1;      // (bin, class) = one counter
    RTUF_LANES(kLaneSetupRecTile, act);
    if (++tx > tx1) { tx = tx0; ty++; }
    unsigned long long mymask = 0;
    int myleader = lane;
    while (pending) {
      const int leader = __ffsll((long long)pending) - 1;
      const int lbin = __builtin_amdgcn_readlane(bin, leader);      // leader is wave-uniform: no LDS crossbar round trip
      const unsigned long long m = __ballot(act && bin == lbin);
      RTUF_LANES(kLaneSetupRecGroup, act && bin == lbin);
      if (act && bin == lbin) { mymask = m; myleader = leader; }
      pending &= ~m;
    }
    uint32_t base = 0;
    if (act && lane == myleader) base = atomicAdd(&a.bin_hdr[bin >> 1].count[cls], (uint32_t)__popcll(mymask));
    // a near record (it may produce window z <= 0.5) marks its bin: top bit of the fragment counter, read by the tile kernel
    const unsigned long long nearm = __ballot(act && (pk.order & kNearBit) != 0u);
    if (nearm && act && lane == myleader && (mymask & nearm)) atomicOr(&a.fbin_count[bin >> 1], 0x80000000u);
    base = __shfl(base, myleader);
    if (act) {
      const uint32_t pos = base + (uint32_t)__popcll(mymask & ((1ull << lane) - 1ull));
      if (pos < a.capacity) store_record(a.bins + (size_t)(bin >> 1) * a.capacity + (cls ? a.capacity - 1u - pos : pos), pk);
      n++;
    }
  }
  return n;
}

// Set-up + coverage of a triangle (snapped coordinates x0..y2 from phase 1) whose pixel-centre bounding box
// is at most N x N (N <= 4): returns
// the covered box positions (bit dy*4+dx, origin bx0,by0) and orients v0/v1 like orient_and_bound.
// All integer work is done relative to the box origin, where vertex coordinates are within
// [-256, (N+1)*256] and every product fits 32 bits (full-rate 24-bit multiplies); the values are
// the same integers the absolute 64-bit form yields.  Straight-line: all N*N candidates per lane.
template <int N>
__device__ __forceinline__ uint32_t small_box_coverage(Win& v0, Win& v1, const Win& v2, int x0, int y0, int x1, int y1, int x2, int y2,
                                                       int width, int height, int& bx0, int& by0)
{
  const int minx = min(x0, min(x1, x2)), maxx = max(x0, max(x1, x2));
  const int miny = min(y0, min(y1, y2)), maxy = max(y0, max(y1, y2));
  bx0 = max((minx + 255) >> 8, 0);
  by0 = max((miny + 255) >> 8, 0);
  const int bx1 = min((maxx - 1) >> 8, width - 1), by1 = min((maxy - 1) >> 8, height - 1);
  if (bx1 < bx0 || by1 < by0) return 0;
  const int ox = bx0 << 8, oy = by0 << 8;
  x0 -= ox; x1 -= ox; x2 -= ox;
  y0 -= oy; y1 -= oy; y2 -= oy;
  const int area = __mul24(x0 - x1, y2 - y0) - __mul24(x2 - x0, y0 - y1);
  if (area == 0) return 0;
  if (area < 0) {
    int t = x0; x0 = x1; x1 = t;
    t = y0; y0 = y1; y1 = t;
    Win tw = v0; v0 = v1; v1 = tw;
  }
  const int xs[3] = {x0, x1, x2}, ys[3] = {y0, y1, y2};
  int A[3], B[3], E[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const int j = (i + 1) % 3;
    const int dcdx = ys[i] - ys[j], dcdy = xs[i] - xs[j];
    int c = __mul24(dcdx, xs[i]) - __mul24(dcdy, ys[i]);
    if (dcdx < 0 || (dcdx == 0 && dcdy > 0)) c += 1;      // (as shifts and subtractions, like edges_from_snapped: 65 instead of 59 registers, 7 waves/SIMD)
    A[i] = -dcdx; B[i] = dcdy;
    E[i] = -((-c) >> 8) - 1;          // inside <=> E + A*dx + B*dy >= 0 (see edges_from_snapped)
  }
  uint32_t out = 0;
#pragma unroll
  for (int dy = 0; dy < N; dy++) {
#pragma unroll
    for (int dx = 0; dx < N; dx++) {
      const int v = (E[0] + dx * A[0] + dy * B[0]) | (E[1] + dx * A[1] + dy * B[1]) | (E[2] + dx * A[2] + dy * B[2]);
      out |= (uint32_t)(~v >> 31 & 1) << (dy * 4 + dx);
    }
  }
  const uint32_t cols = ((2u << (bx1 - bx0)) - 1u) * 0x1111u;
  const uint32_t rows = (uint32_t)((1ull << (4 * (by1 - by0 + 1))) - 1ull);
  return out & cols & rows;
}

// Wave-cooperative emission of the covered pixels of small triangles as 8-byte fragments.  `mask`
// holds the coverage of the box positions (bit dy*4+dx, box origin bx0,by0).  Lanes are grouped by bin
// with ballots, the group leaders reserve popcount(mask) slots each in ONE atomic round trip and
// every lane writes its fragments to consecutive slots.  With MAY_STRADDLE a box whose covered
// positions lie in more than one tile falls back to one plain atomic per fragment.
template <bool MAY_STRADDLE>
__device__ __forceinline__ uint32_t emit_fragments_wave(const SetupArgs& a, int slot, uint32_t mask, int bx0, int by0,
                                                        float a0, float dzdx, float dzdy, uint32_t order)
{
  const int lane = threadIdx.x & 63;
  const int tiles = a.tiles_x * a.tiles_y;
  bool straddle = false;
  if (MAY_STRADDLE) {
    // position dx (dy) lies in the next tile when bx0 % kTileW + dx >= kTileW
    const int rx = kTileW - (bx0 % kTileW), ry = kTileH - (by0 % kTileH);     // positions left in this tile
    const uint32_t colmask = rx >= 4 ? 0xffffu : (((1u << rx) - 1u) * 0x1111u);
    const uint32_t rowmask = ry >= 4 ? 0xffffu : ((1u << (4 * ry)) - 1u);
    straddle = (mask & ~(colmask & rowmask)) != 0;
  }
  const bool act = mask && !straddle;
  const uint32_t cnt = (uint32_t)__popc(mask);
  unsigned long long pending = __ballot(act);
  if (pending) {
    const int bin = act ? __mul24(slot, tiles) + __mul24(by0 / kTileH, a.tiles_x) + (bx0 / kTileW) : -1;
    const unsigned long long c0 = __ballot(act && (cnt & 1u)), c1 = __ballot(act && (cnt & 2u)), c2 = __ballot(act && (cnt & 4u)),
                             c3 = __ballot(act && (cnt & 8u)), c4 = __ballot(act && (cnt & 16u));
    const unsigned long long below = (1ull << lane) - 1ull;
    // The loop only finds every lane's group (the lanes that target the same bin) -- a few instructions per distinct bin.
    // The lane's offset inside its group's reservation and the group's total are then computed ONCE, from the group mask
    // and the five bit planes of the counts (they used to be recomputed inside the loop for every distinct bin: with the
    // three to six bins a wave of small triangles touches, that was most of this function).
    unsigned long long mymask = 0ull;
    int myleader = lane;
    while (pending) {
      const int leader = __ffsll((long long)pending) - 1;
      const int lbin = __builtin_amdgcn_readlane(bin, leader);      // leader is wave-uniform: no LDS crossbar round trip
      const bool mine = act && bin == lbin;
      const unsigned long long m = __ballot(mine);
      RTUF_LANES(kLaneSetupFragGroup, mine);
      if (mine) { mymask = m; myleader = leader; }
      pending &= ~m;
    }
    const unsigned long long lo = mymask & below;
    const uint32_t base_in_group = (uint32_t)(__popcll(c0 & lo) + 2 * __popcll(c1 & lo) + 4 * __popcll(c2 & lo) + 8 * __popcll(c3 & lo) + 16 * __popcll(c4 & lo));
    // the group's total = offset + count of the group's highest lane
    const int top = 63 - __clzll((long long)(mymask | 1ull));
    const uint32_t group_total = (uint32_t)__shfl((int)(base_in_group + cnt), top);
    uint32_t base = 0;
    if (act && lane == myleader) base = atomicAdd(&a.fbin_count[bin], group_total) & 0x7fffffffu;      // (top bit: the bin's near flag)
    base = __shfl(base, myleader);
    if (act) {
      uint32_t pos = base + base_in_group;
      unsigned long long* dst = reinterpret_cast<unsigned long long*>(a.fbins) + (size_t)bin * a.fcapacity;
      const int lbase = (by0 % kTileH) * kTileW + (bx0 % kTileW);
      uint32_t m = mask;
      while (m) {
        RTUF_LANES(kLaneSetupFragStore, true);
        const int k = __ffs((int)m) - 1;
        m &= m - 1;
        const int px = bx0 + (k & 3), py = by0 + (k >> 2);
        if (pos < a.fcapacity) {
          const float z = __fmaf_rn(dzdy, (float)py, __fmaf_rn(dzdx, (float)px, a0));
          // (a triangle that may reach z <= 0.51 anywhere in its box never gets here: it was handed to the record pass)
          const unsigned long long f = ((unsigned long long)z24_of_upper_half(z) << 40) | ((unsigned long long)order << kFragPosBits) |
                                       (unsigned long long)(lbase + (k >> 2) * kTileW + (k & 3));
          dst[pos] = f;
        }
        pos++;
      }
    }
  }
  if (MAY_STRADDLE && straddle) {
    uint32_t m = mask;
    while (m) {
      const int k = __ffs((int)m) - 1;
      m &= m - 1;
      const int px = bx0 + (k & 3), py = by0 + (k >> 2);
      const int bin = __mul24(slot, tiles) + __mul24(py / kTileH, a.tiles_x) + (px / kTileW);
      const uint32_t pos = atomicAdd(&a.fbin_count[bin], 1u) & 0x7fffffffu;
      if (pos < a.fcapacity) {
        const float z = __fmaf_rn(dzdy, (float)py, __fmaf_rn(dzdx, (float)px, a0));
        const unsigned long long f = ((unsigned long long)z24_of_upper_half(z) << 40) | ((unsigned long long)order << kFragPosBits) |
                                     (unsigned long long)((py % kTileH) * kTileW + (px % kTileW));
        reinterpret_cast<unsigned long long*>(a.fbins)[(size_t)bin * a.fcapacity + pos] = f;
      }
    }
  }
  return cnt;
}

// True when the chunk's bounding box lies completely outside frustum plane `plane` (0..5 =
// +x,-x,+y,-y,near,far): then all its vertices carry that plane's clip bit and every triangle
// would be rejected by the per-triangle test anyway (same result, decided once per chunk).
// Margins keep the test conservative.
__device__ __forceinline__ bool chunk_outside_plane(const float* M, const Chunk& ch, int plane)
{
  const int k = plane >> 1;
  const float sg = (plane & 1) ? 1.0f : -1.0f;          // plane: w + sg * coord >= 0
  const float cx = ch.center[0], cy = ch.center[1], cz = ch.center[2];
  const float cw = M[3] * cx + M[7] * cy + M[11] * cz + M[15];
  const float ck = M[k] * cx + M[4 + k] * cy + M[8 + k] * cz + M[12 + k];
  const float nx = M[3] + sg * M[k], ny = M[7] + sg * M[4 + k], nz = M[11] + sg * M[8 + k];
  const float d = cw + sg * ck;
  // the corner of the box farthest along the plane normal is sum |n_i| * half_i above the centre
  const float reach = fabsf(nx) * ch.half[0] + fabsf(ny) * ch.half[1] + fabsf(nz) * ch.half[2];
  const float slack = reach * 1.001f + 1e-5f * (fabsf(cw) + fabsf(ck)) + 1e-30f;
  return d < -slack;
}

// setup_kernel: one workgroup per (chunk, group of kStreamsPerBlock streams).
//   once:        the group's matrices are fetched into LDS; one lane per (stream, frustum plane)
//                decides whether the whole chunk is outside for that stream
//   per stream:  phase 1  every chunk vertex once: vertex shader, clip test, viewport, 1/256-px
//                         snap -> LDS
//                phase 2  one lane per triangle on the snapped integers: trivial reject,
//                         frustum-crossers to the clip list, sub-pixel cull; survivors
//                         (typically < 20 %) are appended to an LDS work list
//   once:        phase 3  the work list of all streams is processed by DENSE waves: full
//                         set-up (edge functions, z plane) and binning
// cull_kernel: one workgroup per chunk, one thread per stream slot of the in-flight group.  Tests
// the chunk's bounding box against the six frustum planes of every stream (plus model selection /
// background mode) and appends the visible streams, kStreamsPerBlock at a time, to the work list
// the set-up kernel runs from.  The test is conservative, so it never changes the image; it only
// keeps ~70 % of the (chunk, stream) pairs of a robot that is partly in view from ever starting a
// set-up workgroup.
static_assert(kStreamsPerBlock <= 4, "WorkItem holds at most 4 stream slots");
__global__ __launch_bounds__(kBlock) void cull_kernel(SetupArgs a)
{
  __shared__ uint16_t s_vis[kBlock];
  __shared__ uint32_t s_wave_n[kBlock / 64];
  __shared__ uint32_t s_base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk_id = blockIdx.x;
  const Chunk ch = a.chunks[chunk_id];
  const bool is_bg = (uint32_t)chunk_id == a.bg_chunk;
  for (int first = 0; first < a.group_size; first += kBlock) {
    const int slot = first + tid;
    bool vis = false;
    if (slot < a.group_size) {
      const int stream = a.group_base + slot;
      vis = is_bg ? (a.bg[stream].mode == 0u) : (((a.model_mask[stream] >> ch.model) & 1ull) != 0ull);
      if (vis) {
        float M[16];
        const float4* src = reinterpret_cast<const float4*>(a.mvp + ((size_t)stream * (a.n_draws + 1) + ch.draw) * 16);
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const float4 col = src[q];
          M[4 * q] = col.x; M[4 * q + 1] = col.y; M[4 * q + 2] = col.z; M[4 * q + 3] = col.w;
        }
#pragma unroll
        for (int pl = 0; pl < 6; pl++) vis = vis && !chunk_outside_plane(M, ch, pl);
      }
    }
    // ordered compaction (wave ballots + a 4-entry prefix): the list order is deterministic
    const unsigned long long vm = __ballot(vis);
    if (lane == 0) s_wave_n[wave] = (uint32_t)__popcll(vm);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; w++) { const uint32_t c = s_wave_n[w]; if (w < wave) before += c; total += c; }
    if (vis) s_vis[before + (uint32_t)__popcll(vm & ((1ull << lane) - 1ull))] = (uint16_t)slot;
    const uint32_t n_items = (total + kStreamsPerBlock - 1) / kStreamsPerBlock;
    if (tid == 0 && n_items) s_base = atomicAdd(&a.counters->work.n_items, n_items);
    __syncthreads();
    if ((uint32_t)tid < n_items) {
      WorkItem it;
      it.chunk = (uint32_t)chunk_id;
      it.tri_begin = ch.tri_begin; it.vert_begin = ch.vert_begin; it.reserved = 0; it.draw = ch.draw;
      it.tri_count = (uint16_t)ch.tri_count; it.vert_count = (uint16_t)ch.vert_count;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t j = (uint32_t)tid * kStreamsPerBlock + k;
        it.slot[k] = (k < kStreamsPerBlock && j < total) ? s_vis[j] : (uint16_t)0xffffu;
      }
      uint4* dst = reinterpret_cast<uint4*>(&a.items[s_base + tid]);
      dst[0] = reinterpret_cast<const uint4*>(&it)[0];
      dst[1] = reinterpret_cast<const uint4*>(&it)[1];
    }
    __syncthreads();
  }
}

// setup_kernel: one workgroup per work item = (chunk, up to kStreamsPerBlock streams that see it).  A chunk is
// <= 256 triangles of one draw call with its own <= kMaxChunkVerts vertex list, so each vertex is transformed
// once per stream (into LDS) instead of once per incident triangle, and the chunk's geometry is loaded
// once for all streams of the item.
// The three survivor lists' counters are fields of ONE LDS word (list_counts, rtuf_numerics.h): a wave reserves in all
// three with one atomic per stream.  (Built with it, measured and taken out again: phase 1 over one index space of all live
// streams' vertices, and the two box classes as one index space -- docs/experiments.md R7.1, docs/patches/setup-dense-experiment.patch.)
static_assert(kStreamsPerBlock * kBlock <= (int)kListFieldMask, "list_counts (rtuf_numerics.h): every list fits its field");

template <bool STRIDED>
__global__ __launch_bounds__(kBlock) void setup_kernel(SetupArgs a, uint32_t item_base)
{
  __shared__ float s_win[kStreamsPerBlock][3][kMaxChunkVerts];  // window x, y, z (SoA: 12 B per vertex)
  __shared__ int2 s_snap[kStreamsPerBlock][kMaxChunkVerts];    // snapped x; snapped y << 8 | clip mask
  __shared__ uint32_t s_packed[kBlock];                         // the chunk's triangles
  __shared__ uint16_t s_list[kStreamsPerBlock * kBlock];        // survivors binned as records: stream k << 8 | triangle
  __shared__ uint16_t s_list2[kStreamsPerBlock * kBlock];       // survivors resolved to fragments: 4x4 boxes from the bottom, 2x2 from the top
  __shared__ uint32_t s_counts;                                 // list_counts(records, 2x2 boxes, 4x4 boxes): the lists' fill
  __shared__ uint32_t s_stat[3];
  __shared__ float s_mvp[kStreamsPerBlock][16];
  __shared__ uint32_t s_on[kStreamsPerBlock];
  __shared__ int s_slot[kStreamsPerBlock];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  if (tid < 3) s_stat[tid] = 0;
  const int shard_id = (int)(blockIdx.x % kCounterShards);
  CounterShard& shard = a.counters->shard[shard_id];
  const float sx = 0.5f * (float)a.width, sy = 0.5f * (float)a.height;
  uint32_t binned = 0, entries = 0, nfrag = 0;
  RTUF_LANES_INIT(0);
  // launch_setup sizes the main grid from the previous batch's work-list length: one item per
  // workgroup (STRIDED = false, no loop: keeps the register count at 8 waves/SIMD).  Items beyond that
  // grid, if the list grew, are swept by a small strided launch of the same code.
  const uint32_t n_items = a.counters->work.n_items;
  // (what this launch covers, for the batch's status word: the main grid takes items [0, gridDim.x); a strided sweep behind
  // it takes everything)
  if (blockIdx.x == 0 && tid == 0) a.counters->work.grid = STRIDED ? 0xffffffffu : gridDim.x;
  for (uint32_t item_id = item_base + blockIdx.x; item_id < n_items; item_id += gridDim.x) {
  if (tid == 3) s_counts = 0;
  // the item carries the chunk's ranges, so the geometry loads depend on it alone
  struct { uint32_t tri_begin, vert_begin, draw, tri_count, vert_count; } ch;
  uint32_t slots01, slots23;
  // The shard whose clip list and many-tile list take this item's triangles comes from the item's CONTENT, not from the
  // workgroup that happens to run it: the cull kernel lists the items in the order its atomics land, so a shard chosen by
  // workgroup index filled differently on every run of the same batch (and a list sized to one run overflowed on the next).
  int list_shard;
  {
    const uint4* src = reinterpret_cast<const uint4*>(&a.items[item_id]);
    uint4 w0 = src[0], w1 = src[1];
    // same address in every lane: move the words to scalar registers so that everything derived
    // from them (ranges, loop bounds, matrix addresses) is wave-uniform for the compiler as well
    w0.x = __builtin_amdgcn_readfirstlane(w0.x); w0.y = __builtin_amdgcn_readfirstlane(w0.y);
    w0.z = __builtin_amdgcn_readfirstlane(w0.z); w0.w = __builtin_amdgcn_readfirstlane(w0.w);
    w1.x = __builtin_amdgcn_readfirstlane(w1.x); w1.y = __builtin_amdgcn_readfirstlane(w1.y);
    w1.z = __builtin_amdgcn_readfirstlane(w1.z); w1.w = __builtin_amdgcn_readfirstlane(w1.w);
    ch.tri_begin = w0.y; ch.vert_begin = w0.z;
    ch.draw = w1.x; ch.tri_count = w1.y & 0xffffu; ch.vert_count = w1.y >> 16;
    slots01 = w1.z; slots23 = w1.w;
    list_shard = (int)((w0.x + (w1.z & 0xffffu)) % (uint32_t)kCounterShards);      // chunk id + first stream slot
  }
  CounterShard& lshard = a.counters->shard[list_shard];
  auto item_slot = [&](int k) { return (int)(((k < 2 ? slots01 : slots23) >> (16 * (k & 1))) & 0xffffu); };

  float4 pv = make_float4(0, 0, 0, 1);
  const bool have_vert = tid < (int)ch.vert_count;
  if (have_vert) pv = a.cverts[ch.vert_begin + tid];
  const bool have_tri = tid < (int)ch.tri_count;
  const uint32_t packed = have_tri ? a.ctris[ch.tri_begin + tid] : 0u;
  s_packed[tid] = packed;
  const uint32_t i0 = packed & 1023u, i1 = (packed >> 10) & 1023u, i2 = (packed >> 20) & 1023u;
  // all matrices of the item's streams are fetched up front (one global round trip per workgroup
  // instead of one per stream) and kept in LDS
  if (tid < kStreamsPerBlock * 16) {
    const int k = tid >> 4, slot = item_slot(k);
    float v = 0.0f;
    if (slot != 0xffff)
      v = a.mvp[((size_t)(a.group_base + slot) * (a.n_draws + 1) + ch.draw) * 16 + (tid & 15)];
    s_mvp[k][tid & 15] = v;
  }
  if (tid >= 64 && tid < 64 + kStreamsPerBlock) {
    const int k = tid - 64;
    s_on[k] = item_slot(k) != 0xffff ? 1u : 0u;
    s_slot[k] = item_slot(k);
  }
  __syncthreads();

  for (int k = 0; k < kStreamsPerBlock; k++) {
    const int slot = s_slot[k];
    if (!s_on[k]) continue;                              // uniform per workgroup
    // (phase 1 of all three streams before ONE barrier, then phase 2 of all three: measured, no difference)
    // phase 1
    RTUF_LANES(kLaneSetupVert, have_vert);
    RTUF_LANES_LIVE(kLaneSetupVertLive, have_vert);
    if (have_vert) {
      float M[16];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const float4 col = reinterpret_cast<const float4*>(s_mvp[k])[q];
        M[4 * q] = col.x; M[4 * q + 1] = col.y; M[4 * q + 2] = col.z; M[4 * q + 3] = col.w;
      }
      float c[4];
      vs_position(M, pv.x, pv.y, pv.z, c);
      const Win w = viewport_vs(c, sx, sy);
      const unsigned cm = clipmask_of(c);
      s_win[k][0][tid] = w.x; s_win[k][1][tid] = w.y; s_win[k][2][tid] = w.z;
      s_snap[k][tid] = make_int2(snap(w.x), (int)(((unsigned)snap(w.y) << 8) | cm));
    }
    __syncthreads();
    // phase 2
    bool survive = false, needs_clip = false, tiny = false, small = false;
    RTUF_LANES(kLaneSetupTri, have_tri);
    if (have_tri) {
      const int2 p0 = s_snap[k][i0], p1 = s_snap[k][i1], p2 = s_snap[k][i2];
      const unsigned m0 = (unsigned)p0.y & 63u, m1 = (unsigned)p1.y & 63u, m2 = (unsigned)p2.y & 63u;
      if ((m0 & m1 & m2) == 0) {
        if ((m0 | m1 | m2) != 0) {
          needs_clip = true;
        } else {
          const int y0 = p0.y >> 8, y1 = p1.y >> 8, y2 = p2.y >> 8;
          const int minx = min(p0.x, min(p1.x, p2.x)), maxx = max(p0.x, max(p1.x, p2.x));
          const int miny = min(y0, min(y1, y2)), maxy = max(y0, max(y1, y2));
          const int bx0 = max((minx + 255) >> 8, 0), bx1 = min((maxx - 1) >> 8, a.width - 1);
          const int by0 = max((miny + 255) >> 8, 0), by1 = min((maxy - 1) >> 8, a.height - 1);
          survive = bx1 >= bx0 && by1 >= by0;
          tiny = survive && (bx1 - bx0) <= 1 && (by1 - by0) <= 1;
          // up to 4x4 candidates inside ONE tile: also resolved to fragments here (boxes that straddle
          // a tile boundary stay records)
          small = survive && !tiny && (bx1 - bx0) <= 3 && (by1 - by0) <= 3 &&
                  (bx0 / kTileW) == (bx1 / kTileW) && (by0 / kTileH) == (by1 / kTileH);
        }
      }
    }
    // triangles that cross a frustum plane go to clip_kernel: one list append per wave
    const unsigned long long cmk = __ballot(needs_clip);
    if (cmk) {
      const int leader = __ffsll((long long)cmk) - 1;
      uint32_t base = 0;
      if (lane == leader) base = atomicAdd(&lshard.clip_count, (uint32_t)__popcll(cmk));
      base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
      if (needs_clip) {
        const uint32_t kk = base + (uint32_t)__popcll(cmk & ((1ull << lane) - 1ull));
        if (kk < a.clip_capacity) {
          uint4* dst = reinterpret_cast<uint4*>(&a.clip_list[(size_t)list_shard * a.clip_capacity + kk]);
          dst[0] = make_uint4((uint32_t)slot, ch.draw, ch.vert_begin, packed);
          dst[1] = make_uint4(a.corder[ch.tri_begin + tid], 0u, 0u, 0u);
        } else {
          lshard.clip_overflow = 1u;
        }
      }
    }
    // survivors go to LDS work lists: records into s_list; boxes resolved to fragments into s_list2
    // (<= 4x4 single-tile boxes from the bottom, <= 2x2 boxes from the top)
    const bool rec = survive && !tiny && !small;
    const unsigned long long sm = __ballot(rec), tm = __ballot(tiny), qm = __ballot(small);
    if (sm | tm | qm) {      // ONE reservation in all three lists: an LDS round trip per wave and stream instead of up to three
      const unsigned long long below = (1ull << lane) - 1ull;
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(&s_counts, list_counts((uint32_t)__popcll(sm), (uint32_t)__popcll(tm), (uint32_t)__popcll(qm)));
      base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
      if (rec) s_list[list_count_rec(base) + (uint32_t)__popcll(sm & below)] = (uint16_t)((k << 8) | tid);
      if (tiny) s_list2[kStreamsPerBlock * kBlock - 1 - (list_count_tiny(base) + (uint32_t)__popcll(tm & below))] = (uint16_t)((k << 8) | tid);
      if (small) s_list2[list_count_small(base) + (uint32_t)__popcll(qm & below)] = (uint16_t)((k << 8) | tid);
    }
  }
  __syncthreads();
  if (RTUF_ABL(a.flags, 0x10000u)) { __syncthreads(); if (!STRIDED) break; continue; }     // timing experiment
  // phase 3a/3b: tiny (2x2) and small (4x4, single tile) survivors -> coverage of their box positions
  // -> 8-byte fragments; the z plane (one division) is only evaluated for triangles that actually
  // cover a pixel centre
  const uint32_t counts = s_counts;
  const uint32_t ntiny = list_count_tiny(counts), nsmall = list_count_small(counts);
  if (tid == 0 && counts == 0u) atomicAdd(&shard.zero_items, 1u);      // (statistics: an item the cull pass could have spared)
  // Dense set-up + binning of one survivor per lane (entry `e` of a work list: stream k << 8 | triangle) as a 32-byte record;
  // the tile kernel rebuilds the edge functions, so only orientation, bounding box and z plane are needed here.  All lanes
  // of a wave call it (emit_record_wave is cooperative); `take`: this lane has an entry.
  auto bin_record = [&](bool take, uint32_t e) {
    bool have = false;
    PackedTri pk;
    uint32_t bbx = 0, bby = 0;
    int slot = 0;
    if (take) {
      const int k = (int)(e >> 8), t = (int)(e & 255u);
      slot = s_slot[k];
      const uint32_t order = a.corder[ch.tri_begin + t];      // (asked for early, see below)
      const uint32_t p = s_packed[t];
      const uint32_t j0 = p & 1023u, j1 = (p >> 10) & 1023u, j2 = (p >> 20) & 1023u;
      Win v0, v1, v2;
      v0.x = s_win[k][0][j0]; v0.y = s_win[k][1][j0]; v0.z = s_win[k][2][j0];
      v1.x = s_win[k][0][j1]; v1.y = s_win[k][1][j1]; v1.z = s_win[k][2][j1];
      v2.x = s_win[k][0][j2]; v2.y = s_win[k][1][j2]; v2.z = s_win[k][2][j2];
      const int2 q0 = s_snap[k][j0], q1 = s_snap[k][j1], q2 = s_snap[k][j2];        // snapped in phase 1 (y << 8 | clip mask)
      int x0 = q0.x, y0 = q0.y >> 8, x1 = q1.x, y1 = q1.y >> 8, x2 = q2.x, y2 = q2.y >> 8, bx0, bx1, by0, by1;
      have = orient_and_bound(v0, v1, v2, a.width, a.height, x0, y0, x1, y1, x2, y2, bx0, bx1, by0, by1);
      if (have) {
        float a0, dzdx, dzdy;
        z_plane(v0, v1, v2, a0, dzdx, dzdy);
        pk = pack_record(x0, y0, x1, y1, x2, y2, a0, dzdx, dzdy, order | near_bit(a0, dzdx, dzdy, bx0, bx1, by0, by1));
        bbx = (uint32_t)bx0 | ((uint32_t)bx1 << 16);
        bby = (uint32_t)by0 | ((uint32_t)by1 << 16);
      }
    }
    RTUF_LANES(kLaneSetupRecHit, have);
    if (__ballot(have) && !RTUF_ABL(a.flags, 0x20000u)) {
      entries += emit_record_wave(a, list_shard, slot, have, bbx, bby, pk);
      binned += have ? 1u : 0u;
    }
  };
#pragma unroll
  for (int cls = 0; cls < 2; cls++) {
    const uint32_t ncls = cls == 0 ? ntiny : nsmall;
    for (uint32_t base = 0; base < ncls; base += kBlock) {
      const uint32_t j = base + tid;
      uint32_t mask = 0;
      int slot = 0, bx0 = 0, by0 = 0;
      float a0 = 0, dzdx = 0, dzdy = 0;
      uint32_t order = 0;
      bool near = false;
      uint32_t ent = 0;
      RTUF_LANES(kLaneSetupSmall, j < ncls);
      RTUF_LANES_LIVE(kLaneSetupSmallLive, j < ncls);
      if (j < ncls) {
        Win v0, v1, v2;
        const uint32_t e = s_list2[cls == 0 ? kStreamsPerBlock * kBlock - 1 - j : j];
        ent = e;
        const int k = (int)(e >> 8), t = (int)(e & 255u);
        slot = s_slot[k];
        // (the draw-order number is asked for right away, not where it is needed: its global-memory latency then passes
        // under the coverage arithmetic instead of after it)
        order = a.corder[ch.tri_begin + t];
        const uint32_t p = s_packed[t];
        const uint32_t j0 = p & 1023u, j1 = (p >> 10) & 1023u, j2 = (p >> 20) & 1023u;
        v0.x = s_win[k][0][j0]; v0.y = s_win[k][1][j0]; v0.z = s_win[k][2][j0];
        v1.x = s_win[k][0][j1]; v1.y = s_win[k][1][j1]; v1.z = s_win[k][2][j1];
        v2.x = s_win[k][0][j2]; v2.y = s_win[k][1][j2]; v2.z = s_win[k][2][j2];
        const int2 q0 = s_snap[k][j0], q1 = s_snap[k][j1], q2 = s_snap[k][j2];      // snapped in phase 1 (y << 8 | clip mask)
        mask = cls == 0 ? small_box_coverage<2>(v0, v1, v2, q0.x, q0.y >> 8, q1.x, q1.y >> 8, q2.x, q2.y >> 8, a.width, a.height, bx0, by0)
                        : small_box_coverage<4>(v0, v1, v2, q0.x, q0.y >> 8, q1.x, q1.y >> 8, q2.x, q2.y >> 8, a.width, a.height, bx0, by0);
        if (mask) {
          z_plane(v0, v1, v2, a0, dzdx, dzdy);
          // z is monotone along x and along y (also as evaluated in float), so its minimum over the box
          // is at a corner.  Anything that may reach window z <= 0.5 needs its plane in the tile
          // kernel (exact float z): it goes out as a record instead (geometry within ~2 x near of the camera).
          // (monotone along each axis: the minimum is at the corner the two slopes point away from)
          const float xm = (float)(dzdx < 0.0f ? bx0 + 3 : bx0), ym = (float)(dzdy < 0.0f ? by0 + 3 : by0);
          const float zmin = __fmaf_rn(dzdy, ym, __fmaf_rn(dzdx, xm, a0));
          near = !(zmin >= 0.51f);      // (a NaN anywhere in the plane makes zmin NaN: counts as near)
        }
      }
      if (near) {      // rare: hand the triangle to the record list (one LDS append: the record field is the packed word's lowest).
        // It lands BEHIND the entries of phase 2, which the record pass below takes without waiting; the tail pass picks it up.
        s_list[list_count_rec(atomicAdd(&s_counts, 1u))] = (uint16_t)ent;
        mask = 0;
      }
      RTUF_LANES(kLaneSetupSmallHit, mask != 0);
      if (__ballot(mask != 0) && !RTUF_ABL(a.flags, 0x40000u)) {
        nfrag += cls == 0 ? emit_fragments_wave<true>(a, slot, mask, bx0, by0, a0, dzdx, dzdy, order)
                          : emit_fragments_wave<false>(a, slot, mask, bx0, by0, a0, dzdx, dzdy, order);
        binned += mask ? 1u : 0u;
      }
    }
  }
  // phase 3c: the larger survivors as records.  No barrier in front of it: the record list as phase 2 left it (`counts`) is
  // complete, and the waves run free.  The list is handed out from the TOP wave downwards: the box passes above fill from
  // wave 0, so the waves that had few boxes or none take the records while the first waves are still in coverage, and the item
  // takes the longer of the two passes instead of their sum (docs/experiments.md R8).
  const uint32_t nlist = list_count_rec(counts);
  for (uint32_t base = 0; base < nlist; base += kBlock) {
    const uint32_t j = base + (uint32_t)(tid ^ (kBlock - 64));
    RTUF_LANES(kLaneSetupRec, j < nlist);
    bin_record(j < nlist, j < nlist ? (uint32_t)s_list[j] : 0u);
  }
  // ... and the tail: what the box passes handed over since (near boxes; none on a robot at arm's length).  The barrier stands
  // where every wave is done with the item anyway.
  __syncthreads();
  const uint32_t nall = list_count_rec(s_counts);
  for (uint32_t base = nlist; base < nall; base += kBlock) {
    const uint32_t j = base + tid;
    RTUF_LANES(kLaneSetupRec, j < nall);
    bin_record(j < nall, j < nall ? (uint32_t)s_list[j] : 0u);
  }
  if (!STRIDED) break;
  __syncthreads();        // LDS is reused by the next item
  }
  // statistics: one (sharded) atomic triple per workgroup
  uint32_t b = binned, e = entries, f = nfrag;
  for (int off = 32; off > 0; off >>= 1) { b += __shfl_down(b, off); e += __shfl_down(e, off); f += __shfl_down(f, off); }
  if (lane == 0 && b) {
    atomicAdd(&s_stat[0], b);
    atomicAdd(&s_stat[1], e);
    atomicAdd(&s_stat[2], f);
  }
  __syncthreads();
  if (tid == 0 && s_stat[0]) {
    atomicAdd(&shard.tris_binned, (unsigned long long)s_stat[0]);
    atomicAdd(&shard.bin_entries, (unsigned long long)s_stat[1]);
    atomicAdd(&shard.frags, (unsigned long long)s_stat[2]);
  }
  RTUF_LANES_FLUSH(shard);
}

// ---------------------------------------------------------------------------------------
// clip_kernel: one thread per triangle that crosses a frustum plane.  Sutherland-Hodgman in
// clip space, planes in the order +x, -x, +y, -y, near, far; each new vertex is interpolated
// from the end point closer to the plane; the polygon is emitted as the fan
// (v[i-1], v[i], v[0]).
// ---------------------------------------------------------------------------------------

__device__ __forceinline__ float clipdist(const float* c, int plane)
{
  // dot4(clip, plane) with planes (-1,0,0,1) (1,0,0,1) (0,-1,0,1) (0,1,0,1) (0,0,1,1) (0,0,-1,1)
  const float px = plane == 0 ? -1.0f : (plane == 1 ? 1.0f : 0.0f);
  const float py = plane == 2 ? -1.0f : (plane == 3 ? 1.0f : 0.0f);
  const float pz = plane == 4 ? 1.0f : (plane == 5 ? -1.0f : 0.0f);
  float s = __fmul_rn(c[0], px);
  s = __fadd_rn(s, __fmul_rn(c[1], py));
  s = __fadd_rn(s, __fmul_rn(c[2], pz));
  s = __fadd_rn(s, c[3]);
  return s;
}

constexpr int kClipBlock = 128;          // threads per clip workgroup (16 KB of LDS polygon storage)
constexpr int kClipMaxV = 16;            // clip-space vertices per triangle: 3 + at most 2 new ones per frustum plane (+1 spare)
constexpr int kClipLdsV = 8;             // ... of which this many live in LDS (a triangle that crosses one or two planes needs 5..7);
                                         // the rest, for the rare triangle that crosses three and more, in a per-thread global spill area
constexpr int kClipGridWgs = 64;         // workgroups per counter shard at most (the spill area is sized for the grid)
constexpr int kClipMaxP = 12;            // polygon vertices (5-bit pool indices packed in one 64-bit register)

// Per-thread polygon clipper.  The vertex pool lives in LDS (thread-interleaved float4s: conflict
// free, no scratch memory) and the two polygon index lists are 5-bit fields of 64-bit registers.
__device__ __forceinline__ int list_get(unsigned long long l, int i) { return (int)((l >> (5 * i)) & 31ull); }

__device__ __forceinline__ void clip_one(const SetupArgs& a, const ClipItem it, int shard_id, float4 (*lds_pool)[kClipBlock], bool valid)
{
  const int t = threadIdx.x;
  float4* const spill = a.clip_spill + (size_t)blockIdx.x * kClipBlock + t;        // [kClipMaxV - kClipLdsV][grid threads]
  const size_t spill_stride = (size_t)gridDim.x * kClipBlock;
  auto pget = [&](int i) -> float4 { return i < kClipLdsV ? lds_pool[i][t] : spill[(size_t)(i - kClipLdsV) * spill_stride]; };
  auto pset = [&](int i, const float4& v) { if (i < kClipLdsV) lds_pool[i][t] = v; else spill[(size_t)(i - kClipLdsV) * spill_stride] = v; };
  const int slot = (int)it.slot, stream = a.group_base + slot;
  const float* __restrict__ M = a.mvp + ((size_t)stream * (a.n_draws + 1) + it.draw) * 16;
  const uint32_t packed = it.packed;
  const uint32_t order = it.order;
  const float sx = 0.5f * (float)a.width, sy = 0.5f * (float)a.height;

  int npool = 3;
  unsigned ormask = 0;
  {
    const uint32_t vi[3] = {packed & 1023u, (packed >> 10) & 1023u, (packed >> 20) & 1023u};
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const float4 p = a.cverts[it.vert_begin + vi[i]];
      float c[4];
      vs_position(M, p.x, p.y, p.z, c);
      lds_pool[i][t] = make_float4(c[0], c[1], c[2], c[3]);
      ormask |= clipmask_of(c);
    }
  }
  unsigned long long inl = 0ull | (1ull << 5) | (2ull << 10), outl = 0;
  int nv = valid ? 3 : 0;
  if (RTUF_ABL(a.flags, 0x200000u)) nv = 0;      // timing experiment: loads and vertex transform only
  unsigned clipmask = ormask;
  bool bad = false;
  while (clipmask && nv >= 3 && !bad) {
    const int plane = __ffs((int)clipmask) - 1;
    clipmask &= ~(1u << plane);
    if (nv >= kClipMaxP) { bad = true; break; }
    int prev = list_get(inl, 0);
    float4 cprev = pget(prev);
    float dp_prev = clipdist(&cprev.x, plane);
    int outc = 0;
    outl = 0;
    for (int i = 1; i <= nv; i++) {
      const int cur = list_get(inl, i == nv ? 0 : i);
      const float4 ccur = pget(cur);
      const float dp = clipdist(&ccur.x, plane);
      bool diff;
      if (dp_prev >= 0.0f) {
        if (outc >= kClipMaxP) { bad = true; break; }
        outl |= (unsigned long long)prev << (5 * outc++);
        diff = dp < 0.0f;
      } else {
        diff = !(dp < 0.0f);
      }
      if (diff) {
        if (npool >= kClipMaxV || outc >= kClipMaxP) { bad = true; break; }
        const float denom = __fsub_rn(dp, dp_prev);
        bool from_cur;
        if (dp < 0.0f) from_cur = dp_prev > -dp;        // going out
        else from_cur = !(dp > -dp_prev);               // coming in
        const float tt = from_cur ? __fdiv_rn(dp, denom) : __fdiv_rn(-dp_prev, denom);
        const float4 o = from_cur ? ccur : cprev;
        const float4 in = from_cur ? cprev : ccur;
        float4 nc;
        nc.x = __fadd_rn(__fmul_rn(__fsub_rn(in.x, o.x), tt), o.x);
        nc.y = __fadd_rn(__fmul_rn(__fsub_rn(in.y, o.y), tt), o.y);
        nc.z = __fadd_rn(__fmul_rn(__fsub_rn(in.z, o.z), tt), o.z);
        nc.w = __fadd_rn(__fmul_rn(__fsub_rn(in.w, o.w), tt), o.w);
        pset(npool, nc);
        outl |= (unsigned long long)npool << (5 * outc++);
        npool++;
      }
      prev = cur;
      cprev = ccur;
      dp_prev = dp;
    }
    inl = outl;
    nv = outc;
  }
  if (bad || nv < 3) nv = 0;           // (all lanes stay for the cooperative emission below)
  if (RTUF_ABL(a.flags, 0x100000u)) nv = 0;      // timing experiment: clip only, emit nothing
  // window coordinates: shaded (original) vertices and clipper-made ones go through different
  // viewport arithmetic (viewport_vs / viewport_clip)
  auto window_of = [&](int idx) {
    const float4 c4 = pget(idx);
    const float c[4] = {c4.x, c4.y, c4.z, c4.w};
    return idx < 3 ? viewport_vs(c, sx, sy) : viewport_clip(c, sx, sy);
  };
  Win w0, wprev;
  if (nv) { w0 = window_of(list_get(inl, 0)); wprev = window_of(list_get(inl, 1)); }
  uint32_t binned = 0, entries = 0;
  // the polygon as a fan (v[i-1], v[i], v[0]); the wave appends its records together (emit_record_wave):
  // the clipped triangles of a stream pile up in the few tiles along the frustum planes, and one
  // reservation per wave and bin instead of one per lane keeps the atomics off each other's cache lines
  for (int i = 2; __ballot(i < nv); i++) {
    bool have = false;
    TriRec r;
    PackedTri pk;
    r.bbx = r.bby = 0;
    if (i < nv) {
      const Win wi = window_of(list_get(inl, i));
      have = make_record(wprev, wi, w0, order, a.width, a.height, r, pk);
      wprev = wi;
    }
    binned += have ? 1u : 0u;
    if (__ballot(have) && !RTUF_ABL(a.flags, 0x800000u)) entries += emit_record_wave(a, shard_id, slot, have, r.bbx, r.bby, pk);      // (0x800000: timing experiment)
  }
  // statistics: one atomic pair per wave (per-lane atomics on a shard's counters serialise at one L2
  // atomic unit -- that alone used to be three quarters of this kernel's time)
  for (int off = 32; off > 0; off >>= 1) { binned += __shfl_down(binned, off); entries += __shfl_down(entries, off); }
  if ((threadIdx.x & 63) == 0 && binned) {
    atomicAdd(&a.counters->shard[shard_id].tris_binned, (unsigned long long)binned);
    atomicAdd(&a.counters->shard[shard_id].bin_entries, (unsigned long long)entries);
  }
}

__global__ __launch_bounds__(kClipBlock) void clip_kernel(SetupArgs a)
{
  __shared__ float4 s_pool[kClipLdsV][kClipBlock];
  // workgroups b, b + kCounterShards, ... serve shard b % kCounterShards
  const int shard_id = blockIdx.x % kCounterShards;
  const uint32_t n = min(a.counters->shard[shard_id].clip_count, a.clip_capacity);
  const uint32_t per = gridDim.x / kCounterShards;
  const ClipItem* list = a.clip_list + (size_t)shard_id * a.clip_capacity;
  // Whole blocks of consecutive list entries per workgroup: neighbours come from the same chunk and stream, so the item,
  // vertex and matrix loads of a wave share cache lines.  (While many-tile records were appended right here, runs of
  // wall triangles had to be dealt out 16 at a time over the workgroups; with bigrec_kernel doing those appends whole
  // blocks are the faster order again.)  Only as many workgroups as the list needs take part: the grid is fixed, the
  // list length lives on the device.
  const uint32_t wg = blockIdx.x / kCounterShards;
  const uint32_t used = min(per, (n + blockDim.x - 1) / blockDim.x);
  if (wg >= used) return;
  for (uint32_t base = 0; base < n; base += used * blockDim.x) {
    const uint32_t i = base + wg * blockDim.x + threadIdx.x;          // whole waves stay in the loop (cooperative emission)
    ClipItem it; it.slot = 0; it.draw = 0; it.vert_begin = 0; it.packed = 0; it.order = 0;
    if (i < n) {
      const uint4* src = reinterpret_cast<const uint4*>(&list[i]);
      const uint4 w0 = src[0];
      it.slot = w0.x; it.draw = w0.y; it.vert_begin = w0.z; it.packed = w0.w; it.order = src[1].x;
    }
    clip_one(a, it, shard_id, s_pool, i < n);
  }
}

// ---------------------------------------------------------------------------------------
// bigrec_kernel: one wave per many-tile record of the shards' lists, in two launches.
//   PHASE 0 (cover)   the wave rebuilds the record's edge functions (uniform work, as in the tile kernel), spreads the
//                     tiles of its bounding box over the lanes and, for every tile the triangle covers COMPLETELY (all
//                     three edge functions positive at their smallest corner of the tile), publishes the largest 24-bit
//                     depth its plane has there: tile_cover[bin] = min over such records of {zmax24, list index}.  No key
//                     of that tile can end up with a larger depth, and the winner of the min becomes the tile's initial
//                     depth keys in the tile kernel (evaluated per pixel there; never walked, never appended).
//   PHASE 1 (append)  drops the tiles the triangle does not touch at all -- an edge function is largest at one corner of
//                     the tile's part of the box; not positive there means no pixel centre of that tile is covered (half
//                     of the tiles of a clipped wall's box) -- and the tiles where the record lies entirely behind the
//                     published cover (its smallest depth over the tile's part of its box is larger: it can win no pixel;
//                     the back of a wall, the wall behind it, the robot's far side behind its own arm), and appends the
//                     record to the back of the others' bins.  Up to four slot reservations per lane are in flight before
//                     the first store needs its answer.
// Exactness: a dropped (record, tile) pair could not have won any depth test of that tile (strictly larger 24-bit depth
// than a fragment that is certainly there), so the keys -- and with them the image -- are the same.
// ---------------------------------------------------------------------------------------
constexpr int kBigWavesPerShard = 64;     // (32 / 128 waves per shard, 2 / 8 reservations in flight per lane: no difference)
template <int PHASE>
__global__ __launch_bounds__(256) void bigrec_kernel(SetupArgs a)
{
  const int lane = threadIdx.x & 63;
  const int wave = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  const int shard_id = wave % kCounterShards, first = wave / kCounterShards;
  CounterShard& shard = a.counters->shard[shard_id];
  const uint32_t count = shard.big_count;
  if (PHASE == 1 && first == 0 && lane == 0 && count > shard.max_big_fill) shard.max_big_fill = count;      // (this wave alone writes the field)
  const uint32_t n = min(count, a.big_capacity);
  const int tiles = a.tiles_x * a.tiles_y;
  uint32_t mine = 0, dropped = 0;
  for (uint32_t j = (uint32_t)first; j < n; j += kBigWavesPerShard) {
    const uint32_t my_id = (uint32_t)shard_id * a.big_capacity + j;
    const BigRec* rec = a.big_list + my_id;
    PackedTri q;
    {
      const uint4* src = reinterpret_cast<const uint4*>(rec);
      uint4* dst = reinterpret_cast<uint4*>(&q);
      dst[0] = src[0]; dst[1] = src[1];
    }
    const int qslot = (int)rec->slot;
    const TriRec r = unpack_record(q, a.width, a.height);
    const int bx0 = (int)(r.bbx & 0xffff), bx1 = (int)(r.bbx >> 16), by0 = (int)(r.bby & 0xffff), by1 = (int)(r.bby >> 16);
    const int tx0 = bx0 / kTileW, tx1 = bx1 / kTileW;
    const int ty0 = by0 / kTileH, ty1 = by1 / kTileH;
    const int tw = tx1 - tx0 + 1, ntile = tw * (ty1 - ty0 + 1);
    if (PHASE == 0) {
      for (int k = lane; k < ntile; k += 64) {
        const int row = k / tw, tx = tx0 + k - row * tw, ty = ty0 + row;
        // the tile's pixels inside the frame
        const int X0 = tx * kTileW, X1 = min(X0 + kTileW, a.width) - 1, Y0 = ty * kTileH, Y1 = min(Y0 + kTileH, a.height) - 1;
        if (bx0 > X0 || bx1 < X1 || by0 > Y0 || by1 < Y1) continue;
        bool inside = true;
#pragma unroll
        for (int e = 0; e < 3; e++) {
          const int xi = r.A[e] > 0 ? X0 : X1, yi = r.B[e] > 0 ? Y0 : Y1;
          inside = inside && (__mul24(r.A[e], xi) + __mul24(r.B[e], yi) + r.C[e]) > 0;
        }
        if (!inside) continue;
        const float zmax = plane_max(r.a0, r.dzdx, r.dzdy, X0, X1, Y0, Y1);
        if (!(zmax == zmax)) continue;
        const int bin = __mul24(qslot, tiles) + __mul24(ty, a.tiles_x) + tx;
        atomicMin(&a.bin_hdr[bin].cover, ((unsigned long long)z24_of(zmax) << 32) | my_id);
        if (q.order & kNearBit) atomicOr(&a.fbin_count[bin], 0x80000000u);      // (a near cover: the tile's keys carry the float's low bits)
      }
      continue;
    }
    constexpr int kPerRound = 4;
    for (int k0 = lane; k0 < ntile; k0 += 64 * kPerRound) {
      int bin[kPerRound];
      uint32_t pos[kPerRound];
#pragma unroll
      for (int jj = 0; jj < kPerRound; jj++) {
        const int k = k0 + 64 * jj;
        bin[jj] = -1;
        pos[jj] = 0;
        if (k < ntile) {
          const int row = k / tw, tx = tx0 + k - row * tw, ty = ty0 + row;
          // the tile's part of the box, in pixel-centre coordinates
          const int x0 = max(bx0, tx * kTileW), x1 = min(bx1, tx * kTileW + kTileW - 1);
          const int y0 = max(by0, ty * kTileH), y1 = min(by1, ty * kTileH + kTileH - 1);
          bool touches = true;
#pragma unroll
          for (int e = 0; e < 3; e++) {
            const int xa = r.A[e] > 0 ? x1 : x0, ya = r.B[e] > 0 ? y1 : y0;
            touches = touches && (__mul24(r.A[e], xa) + __mul24(r.B[e], ya) + r.C[e]) > 0;
          }
          if (touches) {
            const int b = __mul24(qslot, tiles) + __mul24(ty, a.tiles_x) + tx;
            const unsigned long long cv = a.bin_hdr[b].cover;
            if (cv != kNoCover) {
              // this record IS the tile's cover (it becomes the initial keys), or it lies behind the cover everywhere
              const bool behind = z24_of(plane_min(r.a0, r.dzdx, r.dzdy, x0, x1, y0, y1)) > (uint32_t)(cv >> 32);
              if ((uint32_t)cv == my_id || behind) { touches = false; dropped++; }
            }
            if (touches) {
              bin[jj] = b;
              pos[jj] = atomicAdd(&a.bin_hdr[b].count[1], 1u);          // many-tile records are large: back of the bin
              if (q.order & kNearBit) atomicOr(&a.fbin_count[b], 0x80000000u);
              mine++;
            }
          }
        }
      }
#pragma unroll
      for (int jj = 0; jj < kPerRound; jj++)
        if (bin[jj] >= 0 && pos[jj] < a.capacity) store_record(a.bins + (size_t)bin[jj] * a.capacity + (a.capacity - 1u - pos[jj]), q);
    }
  }
  if (PHASE == 0) return;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { mine += (uint32_t)__shfl_down((int)mine, off); dropped += (uint32_t)__shfl_down((int)dropped, off); }
  if (lane == 0 && mine) atomicAdd(&shard.bin_entries, (unsigned long long)mine);
  if (lane == 0 && dropped) atomicAdd(&shard.occluded, (unsigned long long)dropped);
}

// ---------------------------------------------------------------------------------------
// tile_kernel
// ---------------------------------------------------------------------------------------

constexpr unsigned long long kNoFragment = 0x00ffffff00000000ull;   // cleared depth 1.0, order 0
constexpr unsigned long long kResolvedBit = 1ull << 63;


constexpr int kKeyStride = kTileW, kKeyCount = kKeyStride * kTileH;      // the key tile in LDS: one row per pixel row
// MODE 0: depth test (atomicMin of {z24, order});  MODE 1: write the exact float z of the
// fragment that won (needed only for window z <= 0.5, where float z is finer than 24 bits).
// Instrumented builds (-DRTUF_COUNT, scripts/overdraw.sh; never the product): every depth test the tile kernel issues and
// every pixel that ends up drawn is counted through two LDS words per workgroup, summed into the batch's counters.
#ifdef RTUF_COUNT
__device__ __forceinline__ uint32_t* count_words() { __shared__ uint32_t s_cnt[2]; return s_cnt; }
#define RTUF_COUNT_TEST() atomicAdd(&count_words()[0], 1u)
#else
#define RTUF_COUNT_TEST() ((void)0)
#endif

// Depth keys: {z24, draw order << shift | low bits of the fragment's float z}.  The draw order takes as many of the low
// word's bits as the context's triangle count needs (shift = 32 - those), the rest carries the LOW BITS OF THE FLOAT Z in
// tiles that hold near geometry: the shader sees the unquantised gl_FragCoord.z, which below window z 0.5 is finer than
// the 24-bit depth that decides the test -- but z24 pins z to an interval of 2^-24, and the float's low `shift` bits single
// out one float in it as long as the interval holds fewer than 2^(shift-1) floats, i.e. for z24 >= 2^(26-shift)
// (near_z_from_key; checked exhaustively on the CPU, tests/test_near_keys_cpu.py).  The low bits sit below the draw
// order, and a triangle meets a pixel once, so they never decide a comparison: atomicMin still is "nearest 24-bit depth,
// first drawn wins ties".  Round 3 re-walked every near record of such a tile to fetch the winners' float z (24,048 of
// 38,400 tiles with the arm in front of the lens); now only winners closer than z24 < zexact still need that pass
// (15 um in front of the near plane for the 250 k-triangle model).
struct KeyFmt {
  int shift;            // draw order << shift in the key's low word (TileArgs::key_shift)
  uint32_t lowmask;     // (1 << shift) - 1 in tiles that hold near records (or a near cover), else 0
  uint32_t zexact;      // winners with z24 < zexact need the exact-z pass: 2^(26-shift) in near tiles, else 2^23 + 1
  uint32_t abl;         // RTUF_ABLATE builds: the launch's timing-experiment bits (0x4000: depth tests without their LDS atomic, 0x2000000: strips fetched but not walked)
  bool keep_order;      // link labels (a compile-time constant of the kernel): resolved keys keep the winner's draw order
};

// The exact-z pass replaces a winning key by kResolvedBit | float z.  Bits 32-62 of that word are unused; with link labels they
// keep the winner's draw order (at most 29 bits, kMaxOrder), which the label lookup needs.  (keep_order is false in every
// kernel without labels, so there this is the same single OR it always was.)
__device__ __forceinline__ unsigned long long resolved_key(unsigned long long key, float z, const KeyFmt& kf)
{
  const unsigned long long ord = kf.keep_order ? (unsigned long long)((uint32_t)key >> kf.shift) << 32 : 0ull;
  return kResolvedBit | ord | (unsigned long long)__float_as_uint(z);
}
// draw order of a resolved key (keep_order)
__device__ __forceinline__ uint32_t resolved_order(unsigned long long k) { return (uint32_t)(k >> 32) & 0x7fffffffu; }
// The winner's draw order: the key's, or -- after the exact-z pass -- the one resolved_key kept above the float z.  0 is "no
// fragment" (kNoFragment), whose label table entry is 0, and the background quad drawn as geometry, whose threshold table entry
// is max_diff.
__device__ __forceinline__ uint32_t winner_order(unsigned long long k, const KeyFmt& kf) { return (k & kResolvedBit) ? resolved_order(k) : (uint32_t)k >> kf.shift; }

// One depth test of a fragment whose window z is already evaluated (`order`: the draw order shifted into place).
// Issue classes (profiles/valu_peak.json: gfx950 issues v_fma/mul/add_f32, v_add/sub_u32, v_and/or/xor_b32 and the right shifts
// in 2 cycles per wave64, everything else -- conversions, v_rndne, min/max, compares, selects, 24-bit multiplies, left shifts --
// in 4): the hot walks use 2-cycle ones wherever they compute the same number (z24_of_upper_half, rtuf_numerics.h).
template <int MODE, bool LOW>
__device__ __forceinline__ void depth_test(unsigned long long* keys, uint32_t order, float z, int lidx, const KeyFmt& kf, int lc)
{
  if (MODE == 0) RTUF_COUNT_TEST();
  if (MODE == 0) RTUF_LANES(lc, true);
  const uint32_t lo = LOW ? (order | (__float_as_uint(z) & kf.lowmask)) : order;
  const unsigned long long key = ((unsigned long long)((!LOW && MODE == 0) ? z24_of_upper_half(z) : z24_of(z)) << 32) | lo;
  if (RTUF_ABL(kf.abl, 0x4000u)) { if (key == 0x0123456789abcdefull) keys[lidx] = key; return; }      // timing experiment: everything but the atomic
  if (MODE == 0) {
    atomicMin(&keys[lidx], key);
  } else {
    if (keys[lidx] == key) keys[lidx] = resolved_key(key, z, kf);
  }
}

template <int MODE, bool LOW>
__device__ __forceinline__ void fragment(unsigned long long* keys, const TriRec& r, int px, int py, int lidx, const KeyFmt& kf, int lc = kLaneWalkFrag)
{
  // (r.order holds the draw order already shifted into place)
  depth_test<MODE, LOW>(keys, r.order, __fmaf_rn(r.dzdy, (float)py, __fmaf_rn(r.dzdx, (float)px, r.a0)), lidx, kf, lc);
}


#ifndef RTUF_SMALL_AREA
#define RTUF_SMALL_AREA 96
#endif
#ifndef RTUF_QUARTER_AREA
#define RTUF_QUARTER_AREA 256
#endif
constexpr int kSmallArea = RTUF_SMALL_AREA;     // bounding boxes up to this many pixels are walked by their own lane
#ifndef RTUF_PARK_BELOW
#define RTUF_PARK_BELOW 128
#endif
#ifndef RTUF_WALL_AREA
#define RTUF_WALL_AREA 1536
#endif
constexpr int kWallArea = RTUF_WALL_AREA;         // ... larger bins only for boxes covering more of the tile than this
constexpr int kParkBelow = RTUF_PARK_BELOW;       // bins of at most this many records use the cooperative whole-tile pass
constexpr int kHugeMax = 127;
// Exact-z pass: which draw-order keys won a pixel that needs its exact float z -- a 4096-bit filter in LDS (one multiplicative
// hash); records whose key is not in it cannot be a winner and are not walked a second time.
constexpr int kWinnerWords = 128;
__device__ __forceinline__ uint32_t winner_slot(uint32_t order) { return (order * 0x9E3779B1u) >> 20; }      // 12 bits
constexpr int kQuarterArea = RTUF_QUARTER_AREA;   // up to this many by a quarter wave (4 triangles at a time), larger by the whole wave

// The tile's part of a record's box (local lx0..ly1) against the three edges: an edge function is largest /
// smallest at a corner.  Not positive at its largest for some edge: no pixel centre of this tile is covered
// (half of the tiles of a screen-filling triangle's box) -> returns 0.  Positive at its smallest for all
// three: every candidate is covered -> returns 2 (no edge tests needed).  Otherwise 1.
__device__ __forceinline__ int classify_box(const TriRec& r, int x_base, int y_base, int lx0, int lx1, int ly0, int ly1)
{
  bool reject = false, inside = true;
#pragma unroll
  for (int e = 0; e < 3; e++) {
    const int xa = x_base + (r.A[e] > 0 ? lx1 : lx0), xi = x_base + (r.A[e] > 0 ? lx0 : lx1);
    const int ya = y_base + (r.B[e] > 0 ? ly1 : ly0), yi = y_base + (r.B[e] > 0 ? ly0 : ly1);
    reject = reject || (__mul24(r.A[e], xa) + __mul24(r.B[e], ya) + r.C[e]) <= 0;
    inside = inside && (__mul24(r.A[e], xi) + __mul24(r.B[e], yi) + r.C[e]) > 0;
  }
  return reject ? 0 : (inside ? 2 : 1);
}

// Broadcast of one lane's record to the whole wave through scalar registers (v_readlane): the
// cooperative path then runs with the triangle's 16 words as SGPR operands.
__device__ __forceinline__ TriRec broadcast_record(const TriRec& r, int src_lane)
{
  TriRec q;
  const int* s = reinterpret_cast<const int*>(&r);
  int* d = reinterpret_cast<int*>(&q);
#pragma unroll
  for (int k = 0; k < 16; k++) d[k] = __builtin_amdgcn_readlane(s[k], src_lane);
  return q;
}

// One lane's step of the cooperative paths: pixel (lx, ly) of the tile and the one below it (limited to the
// box, qy1 inclusive).  Neighbouring lanes take neighbouring columns, so each of the two LDS atomics of a
// step is conflict-free across the wave; the lower pixel's edge values are the upper one's plus B.
template <int MODE, bool LOW>
__device__ __forceinline__ void raster_pair(unsigned long long* keys, const TriRec& q, int x_base, int y_base, int lx, int ly, int qy1, const KeyFmt& kf, int lc = kLaneQuarterFrag)
{
  const int px = x_base + lx, py = y_base + ly;
  const int e0 = __mul24(q.A[0], px) + __mul24(q.B[0], py) + q.C[0];
  const int e1 = __mul24(q.A[1], px) + __mul24(q.B[1], py) + q.C[1];
  const int e2 = __mul24(q.A[2], px) + __mul24(q.B[2], py) + q.C[2];
  const int lidx = ly * kKeyStride + lx;
  if (min(e0, min(e1, e2)) > 0) fragment<MODE, LOW>(keys, q, px, py, lidx, kf, lc);
  if (min(e0 + q.B[0], min(e1 + q.B[1], e2 + q.B[2])) > 0 && ly < qy1) fragment<MODE, LOW>(keys, q, px, py + 1, lidx + kKeyStride, kf, lc);
}

// Row-stepped walk of a strip -- columns qx0 .. qx0 + wc - 1 (wc <= 2^team_log) of the record's part of the tile, rows qy0 ..
// qy0 + h - 1 -- by a TEAM of 2^team_log lanes (`sub` = the lane's number in its team).  The team forms 2^plog columns (the
// power of two that holds wc) x 2^lr rows; every lane keeps its column and steps DOWN the rows, 2^lr at a time, two steps per
// trip.  Nothing is evaluated per candidate but what changes: the three edge values move by B << lr per step (integer adds
// modulo 2^32 of the same integers A*px + B*py + C is made of -- the value at a pixel is the same number whichever way it is
// reached), the plane's column term fma(dzdx, px, a0) is the lane's constant and the row's float coordinate moves by 2^lr (small
// integers: exact), so fma(dzdy, py, .) sees the operands fragment() gives it.  A trip costs 16 VALU instructions for 2 x 2^team_log
// candidates where the linear run of pairs it replaces (raster_pair: index -> column / row by a reciprocal multiply, six 24-bit
// multiplies per pair) took 42.  EDGES = false: the caller knows that every candidate is covered (classify_box == 2).
template <int MODE, bool LOW, bool EDGES>
__device__ __forceinline__ void strip_walk(unsigned long long* keys, const TriRec& q, int x_base, int y_base, int qx0, int wc, int qy0, int h,
                                           int team_log, int sub, bool on, const KeyFmt& kf, int lc_trip, int lc_frag)
{
  const int plog = wc > 1 ? 32 - __clz(wc - 1) : 0, lr = team_log - plog;
  const int col = sub & ((1 << plog) - 1), row0 = sub >> plog;
  // rows row0, row0 + 2^lr, ... below h (row0 < 2^lr: the numerator is never negative)
  int nrow = (on && col < wc) ? (h - 1 - row0 + (1 << lr)) >> lr : 0;
  const int px = x_base + qx0 + col, py = y_base + qy0 + row0;
  int e0 = 1, e1 = 1, e2 = 1, d0 = 0, d1 = 0, d2 = 0;
  if (EDGES) {
    e0 = __mul24(q.A[0], px) + __mul24(q.B[0], py) + q.C[0];
    e1 = __mul24(q.A[1], px) + __mul24(q.B[1], py) + q.C[1];
    e2 = __mul24(q.A[2], px) + __mul24(q.B[2], py) + q.C[2];
    d0 = (int)((uint32_t)q.B[0] << lr); d1 = (int)((uint32_t)q.B[1] << lr); d2 = (int)((uint32_t)q.B[2] << lr);
  }
  const float zc = __fmaf_rn(q.dzdx, (float)px, q.a0);
  float fy = (float)py;
  const float dfy = (float)(1 << lr);
  int lidx = (qy0 + row0) * kKeyStride + qx0 + col;
  const int dl = kKeyStride << lr;
  while (__ballot(nrow > 0)) {
    if (MODE == 0) RTUF_LANES(lc_trip, nrow > 0);
    const int f0 = e0 + d0, f1 = e1 + d1, f2 = e2 + d2;
    if (nrow > 0 && (!EDGES || min(e0, min(e1, e2)) > 0)) depth_test<MODE, LOW>(keys, q.order, __fmaf_rn(q.dzdy, fy, zc), lidx, kf, lc_frag);
    if (nrow > 1 && (!EDGES || min(f0, min(f1, f2)) > 0)) depth_test<MODE, LOW>(keys, q.order, __fmaf_rn(q.dzdy, __fadd_rn(fy, dfy), zc), lidx + dl, kf, lc_frag);
    e0 = f0 + d0; e1 = f1 + d1; e2 = f2 + d2;
    fy = __fadd_rn(fy, __fadd_rn(dfy, dfy));
    lidx += 2 * dl;
    nrow -= 2;
  }
}

// Rasterises the bin's records into the LDS key tile.  Every wave works on the records it loaded:
// lane-per-triangle for small bounding boxes, a quarter wave each for the middle class; triangles
// that cover a large part of the tile are parked and, after one workgroup barrier at the end, walked
// by all waves together (all threads of the workgroup must call this function).
// `zcover` is the tile's occlusion bound (24-bit depth no key of the tile can exceed; 0xffffffff = none, wave-uniform): records
// that lie behind it over their whole part of the tile are dropped when they are loaded.  MODE 1 looks only at records the
// set-up marked as near (kNearBit) and, of those, only at the ones that can reach the lower half of the depth range here.

template <int MODE, bool LOW, int NT>
__device__ __forceinline__ void raster_bin(unsigned long long* keys, const PackedTri* recs, uint32_t n,
                                           int x_base, int y_base, int tid, bool dbg_load_only, int width, int height, uint32_t n_front, uint32_t capacity,
                                           uint32_t* s_huge, TriRec* s_prec, uint4* s_pmeta, uint32_t zcover, const uint32_t* s_winners, const KeyFmt& kf,
                                           uint4 first0, uint4 first1, bool have_first, int dbg_skip = 0)
{
  const int lane = tid & 63;
  const uint32_t zdrop = MODE == 1 ? min(zcover, kf.zexact - 1u) : zcover;      // MODE 1: only what can reach a depth that needs the pass
  // (round 5 measured two ways of balancing the walks here and took both out again: windows sorted by box size, branch
  // sorted-walk-experiment -- fewer trips, slower for its barriers; records behind the cover compacted through a per-wave queue
  // before the unpack, branch cover-compaction-experiment -- fuller waves, slower for its second load.  DESIGN.md A.5)
  for (uint32_t base = 0; base < n; base += NT) {
    const uint32_t i = base + tid;
    bool have = i < n;
    const uint32_t ri = i < n_front ? i : capacity - 1u - (i - n_front);      // small boxes from the front, larger ones from the back
    const bool first_in_regs = have_first && base == 0u;
    TriRec r;
    int lx0 = 0, lx1 = -1, ly0 = 0, ly1 = -1;
    PackedTri pk;
    if (MODE == 0) RTUF_LANES(kLaneTileLoad, have);
    if (have) {
      uint4* dst = reinterpret_cast<uint4*>(&pk);
      if (first_in_regs) {
        dst[0] = first0; dst[1] = first1;      // (the caller asked for this lane's first record before it initialised the key tile)
      } else {
        const uint4* src = reinterpret_cast<const uint4*>(recs + ri);
        dst[0] = src[0]; dst[1] = src[1];
      }
      if (MODE == 1) {          // only near records whose draw-order key won a pixel that needs resolving
        const uint32_t h = winner_slot(pk.order & kOrderMask);
        if (!(pk.order & kNearBit) || !((s_winners[h >> 5] >> (h & 31u)) & 1u)) have = false;
      }
    }
    if (have) {
      r = unpack_record(pk, width, height);
      r.order <<= kf.shift;
      lx0 = max((int)(r.bbx & 0xffff) - x_base, 0);
      lx1 = min((int)(r.bbx >> 16) - x_base, kTileW - 1);
      ly0 = max((int)(r.bby & 0xffff) - y_base, 0);
      ly1 = min((int)(r.bby >> 16) - y_base, kTileH - 1);
    } else {
#pragma unroll
      for (int q = 0; q < 16; q++) reinterpret_cast<int*>(&r)[q] = 0;
    }
    const int w = lx1 - lx0 + 1, h = ly1 - ly0 + 1;
    int area = (have && w > 0 && h > 0) ? w * h : 0;
    if (zdrop != 0xffffffffu) {               // (uniform) behind the tile's cover / out of the exact-z range: cannot matter here
      if (area > 0 && z24_of(plane_min(r.a0, r.dzdx, r.dzdy, x_base + lx0, x_base + lx1, y_base + ly0, y_base + ly1)) > zdrop) area = 0;
    }
    if (dbg_load_only) { if (r.order == 0xdeadbeefu) keys[0] = 0; area = 0; }
    if (dbg_skip == 1 && area <= kSmallArea) area = 0;      // timing experiment: no lane-per-triangle walk
    if (dbg_skip == 2 && area > kSmallArea) area = 0;       // timing experiment: no quarter-wave walk
    if (dbg_skip == 3 && area > kQuarterArea) area = 0;     // timing experiment: no whole-tile walks
    const bool small = area > 0 && area <= kSmallArea;
#ifdef RTUF_LANECOUNT
    if (MODE == 0 && have) {
      const int td = ((lx1 - lx0 + 2) >> 1) * ((ly1 - ly0 + 2) >> 1);
      const int b = area <= 0 ? kLaneHistNone : (area > kQuarterArea ? kLaneHistLarge : (area > kSmallArea ? kLaneHistQuarter :
                    kLaneHist + (td <= 6 ? td - 1 : (td <= 8 ? 6 : (td <= 12 ? 7 : (td <= 16 ? 8 : (td <= 24 ? 9 : 10)))))));
      atomicAdd(&lane_words()[2 * b + 1], 1u);
      const int fw = (int)(r.bbx >> 16) - (int)(r.bbx & 0xffff) + 1, fh = (int)(r.bby >> 16) - (int)(r.bby & 0xffff) + 1;
      const bool one_tile = (int)(r.bbx & 0xffff) / kTileW == (int)(r.bbx >> 16) / kTileW && (int)(r.bby & 0xffff) / kTileH == (int)(r.bby >> 16) / kTileH;
      if (one_tile && fw <= 8 && fh <= 8 && !(pk.order & kNearBit)) atomicAdd(&lane_words()[2 * kLaneHist8x8 + 1], 1u);
      if (one_tile && ((fw <= 8 && fh <= 4) || (fw <= 4 && fh <= 8)) && !(pk.order & kNearBit)) atomicAdd(&lane_words()[2 * kLaneHist8x4 + 1], 1u);
    }
#endif
    // lane-per-triangle: walk the bounding box as one run of 2x2 candidate QUADS, quad row by quad row.
    // The three edge values of a quad's upper left pixel are stepped incrementally (one add each, a
    // different step at the end of a quad row); the other three pixels' are those plus A, B, A + B -- the
    // same integer arithmetic as evaluating A*px + B*py + C at every candidate, at about half the
    // instructions per candidate and a quarter of the loop trips.
    {
      // The pixel position is kept as two floats (small integers: every add is exact) -- the plane wants them as floats, and
      // four conversions per trip would be 4-cycle instructions; the key's LDS address is stepped in bytes (no left shift per
      // trip); the right-hand pixels of a quad lie outside the box only in the last quad column of a box of odd width, which
      // the wrap test already knows (one compare less: tests/fast_class_check.cpp).
      const int qcols = (lx1 - lx0 + 2) >> 1;                              // quads per quad row
      const int back = 2 * (qcols - 1);                                    // x distance from the last quad of a row to the first
      const float fpx0 = (float)(x_base + lx0), fpy_last = (float)(y_base + ly1), fpx_lastq = (float)(x_base + lx0 + back);
      float fpx = fpx0, fpy = (float)(y_base + ly0);
      uint32_t kofs = (uint32_t)(ly0 * kKeyStride + lx0) * 8u;             // byte offset of the quad's upper left key
      int e0 = __mul24(r.A[0], x_base + lx0) + __mul24(r.B[0], y_base + ly0) + r.C[0];
      int e1 = __mul24(r.A[1], x_base + lx0) + __mul24(r.B[1], y_base + ly0) + r.C[1];
      int e2 = __mul24(r.A[2], x_base + lx0) + __mul24(r.B[2], y_base + ly0) + r.C[2];
      // a step to the right always; the lanes at the end of a quad row then add what takes them to the start of the next one
      // (five 2-cycle adds under the wrap's lane mask instead of six selects)
      const int a0x2 = 2 * r.A[0], a1x2 = 2 * r.A[1], a2x2 = 2 * r.A[2];
      const int d0 = 2 * r.B[0] - __mul24(back + 2, r.A[0]), d1 = 2 * r.B[1] - __mul24(back + 2, r.A[1]), d2 = 2 * r.B[2] - __mul24(back + 2, r.A[2]);
      const uint32_t dk = (uint32_t)(2 * kKeyStride - back - 2) * 8u;
      const bool odd_w = ((lx1 - lx0) & 1) == 0;                           // the last quad column holds one pixel column
      int todo = small ? __mul24(qcols, (ly1 - ly0 + 2) >> 1) : 0;
      auto test = [&](float x, float y, uint32_t ofs) {
        depth_test<MODE, LOW>(reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(keys) + ofs), r.order,
                              __fmaf_rn(r.dzdy, y, __fmaf_rn(r.dzdx, x, r.a0)), 0, kf, kLaneWalkFrag);
      };
      while (__ballot(todo > 0)) {
        if (MODE == 0) RTUF_LANES(kLaneWalkTrip, todo > 0);
        if (todo > 0) {
          const bool wrap = fpx == fpx_lastq;
          const bool no_right = wrap && odd_w, below = fpy < fpy_last;
          const int f0 = e0 + r.B[0], f1 = e1 + r.B[1], f2 = e2 + r.B[2];
          const float fx1 = __fadd_rn(fpx, 1.0f), fy1 = __fadd_rn(fpy, 1.0f);
          if (min(e0, min(e1, e2)) > 0) test(fpx, fpy, kofs);
          if (min(e0 + r.A[0], min(e1 + r.A[1], e2 + r.A[2])) > 0 && !no_right) test(fx1, fpy, kofs + 8u);
          if (min(f0, min(f1, f2)) > 0 && below) test(fpx, fy1, kofs + 8u * kKeyStride);
          if (min(f0 + r.A[0], min(f1 + r.A[1], f2 + r.A[2])) > 0 && !no_right && below) test(fx1, fy1, kofs + 8u * kKeyStride + 8u);
          e0 += a0x2; e1 += a1x2; e2 += a2x2;
          kofs += 16u;
          fpx = __fadd_rn(fpx, 2.0f);
          todo--;
          if (wrap) {
            asm volatile("" ::: "memory");      // (keeps this a masked block: as selects it is six 4-cycle instructions)
            e0 += d0; e1 += d1; e2 += d2;
            kofs += dk;
            fpy = __fadd_rn(fpy, 2.0f);
            fpx = fpx0;
          }
        }
      }
    }
    // quarter-wave cooperative: four triangles at a time, 16 lanes each, one vertical candidate pair per
    // lane and step (the bounding box is walked as a linear run of pairs, so slivers waste little)
    // whole-wave cooperative: triangles that cover a large part of the tile, one at a time with the
    // record in scalar registers (v_readlane), 64 candidate pairs per step
    unsigned long long huge = __ballot(area > kQuarterArea);
    if (huge) {
      // those whose triangle misses this tile altogether drop out here
      huge &= ~__ballot(area > kQuarterArea && classify_box(r, x_base, y_base, lx0, lx1, ly0, ly1) == 0);
    }
    const unsigned long long park = huge ? (huge & __ballot(area > (int)s_huge[1 + kHugeMax])) : 0ull;
    if (park) {
      // In a bin that one or two waves hold alone (typical: a few walls) all of them, in fuller bins only those
      // that cover nearly the whole tile (the kernel puts the area threshold behind the list) are parked in
      // the workgroup's list (s_huge[0] = count, then bin indices): after this loop all four waves rasterise
      // each of them together.  Otherwise every wave has its own, and walking them alone avoids paying each
      // triangle's fixed cost four times.  What does not fit the list stays with this wave, too.
      const int leader = __ffsll((long long)park) - 1;
      uint32_t hb = 0;
      if (lane == leader) hb = atomicAdd(&s_huge[0], (uint32_t)__popcll(park));
      hb = (uint32_t)__builtin_amdgcn_readlane((int)hb, leader);
      const uint32_t hs = hb + (uint32_t)__popcll(park & ((1ull << lane) - 1ull));
      const bool parked = ((park >> lane) & 1ull) != 0 && hs < (uint32_t)kHugeMax;
      if (parked) s_huge[1 + hs] = ri;
      huge &= ~__ballot(parked);
    }
    if constexpr (LOW || MODE == 1) {
    // Everything beyond the lane-per-triangle class that stays with this wave: STRIPS, one per team of lanes.  A strip is up to
    // 16 columns of a record's part of the tile over all its rows (a wider record is dealt out as two to four strips, to
    // neighbouring teams or successive rounds); its lanes step down the rows (strip_walk).  With three and more records waiting
    // a round deals four strips to the four quarters of the wave; the last two share the wave half and half, a single one gets
    // all 64 lanes (16 columns x 4 rows per step).  The record travels from the lane that loaded it with 15 shuffles.
    // Taken in tiles with near geometry only (the LOW instance and the exact-z pass), where such records
    // come by the dozen per wave-load and the rounds are full: tile kernel 1.117 -> 1.07 ms with the arm in front of the lens.
    // Elsewhere a wave-load holds one such record in four, a round is one strip, and the pair runs below measure the same or
    // better (C3 +0.5 %, C4 / C5 shares +-0.5 %: profiles/r05_experiment_strips.txt).
    {
      unsigned long long big = __ballot(area > kSmallArea && (area <= kQuarterArea || ((huge >> lane) & 1ull) != 0ull));
      const int nstrip = (lx1 - lx0 + 16) >> 4;
      int head_strip = 0;                      // (scalar) the next strip of the record at the head of `big`
      while (big) {
        const int waiting = __popcll(big);
        const int team_log = waiting >= 3 ? 4 : (waiting == 2 ? 5 : 6);      // (scalar)
        const int grp = lane >> team_log, sub = lane & ((1 << team_log) - 1);
        int src = -1, strip = 0;
#pragma unroll
        for (int g = 0; g < 4; g++) {
          if (g < (64 >> team_log)) {
            const int sl = big ? __ffsll((long long)big) - 1 : -1;
            const int si = head_strip;
            if (big) {
              if (++head_strip >= __builtin_amdgcn_readlane(nstrip, sl)) { big &= big - 1; head_strip = 0; }
            }
            if (g == grp) { src = sl; strip = si; }
          }
        }
        const int srcl = src < 0 ? lane : src;
        TriRec q;
        {
          const int* sp = reinterpret_cast<const int*>(&r);
          int* dp = reinterpret_cast<int*>(&q);
#pragma unroll
          for (int k = 0; k < 15; k++) dp[k] = __shfl(sp[k], srcl);
        }
        const int qx0 = max((int)(q.bbx & 0xffff) - x_base, 0) + 16 * strip, qx1 = min((int)(q.bbx >> 16) - x_base, kTileW - 1);
        const int qy0 = max((int)(q.bby & 0xffff) - y_base, 0), qy1 = min((int)(q.bby >> 16) - y_base, kTileH - 1);
        if (RTUF_ABL(kf.abl, 0x2000000u)) { if (q.order == 0xdeadbeefu) keys[0] = 0; continue; }      // timing experiment: strips dealt out and fetched, not walked
        strip_walk<MODE, LOW, true>(keys, q, x_base, y_base, qx0, min(qx1 - qx0 + 1, 16), qy0, qy1 - qy0 + 1, team_log, sub, src >= 0, kf, kLaneQuarterTrip, kLaneQuarterFrag);
      }
    }
    } else {
    const int grp = lane >> 4, sub = lane & 15;
    while (huge) {
      const int src = __ffsll((long long)huge) - 1;
      huge &= huge - 1;
      const TriRec q = broadcast_record(r, src);
      const int qx0 = max((int)(q.bbx & 0xffff) - x_base, 0), qx1 = min((int)(q.bbx >> 16) - x_base, kTileW - 1);
      const int qy0 = max((int)(q.bby & 0xffff) - y_base, 0), qy1 = min((int)(q.bby >> 16) - y_base, kTileH - 1);
      // the box as a linear run of vertical pixel pairs, one pair per lane and step
      const int qw = qx1 - qx0 + 1, npair = qw * ((qy1 - qy0 + 2) >> 1);
      const uint32_t inv = (uint32_t)ceilf(1048576.0f * __builtin_amdgcn_rcpf((float)qw));
      for (int idx = lane; idx < npair; idx += 64) {
        if (MODE == 0) RTUF_LANES(kLaneWaveTrip, true);
        const int yy = (int)((uint32_t)__mul24(idx, (int)inv) >> 20);
        raster_pair<MODE, LOW>(keys, q, x_base, y_base, qx0 + idx - __mul24(yy, qw), qy0 + 2 * yy, qy1, kf, kLaneWaveFrag);
      }
    }
    unsigned long long big = __ballot(area > kSmallArea && area <= kQuarterArea);
    while (big) {
      int src = -1;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const int sl = big ? __ffsll((long long)big) - 1 : -1;
        if (big) big &= big - 1;
        if (g == grp) src = sl;
      }
      const int srcl = src < 0 ? lane : src;
      TriRec q;
      {
        const int* sp = reinterpret_cast<const int*>(&r);
        int* dp = reinterpret_cast<int*>(&q);
#pragma unroll
        for (int k = 0; k < 15; k++) dp[k] = __shfl(sp[k], srcl);
      }
      const int qx0 = max((int)(q.bbx & 0xffff) - x_base, 0), qx1 = min((int)(q.bbx >> 16) - x_base, kTileW - 1);
      const int qy0 = max((int)(q.bby & 0xffff) - y_base, 0), qy1 = min((int)(q.bby >> 16) - y_base, kTileH - 1);
      const int qw = qx1 - qx0 + 1;
      const int npair = src < 0 ? 0 : qw * ((qy1 - qy0 + 2) >> 1);
      // idx / qw for idx < 4096, qw <= 128 via a reciprocal multiply that is exact in that range:
      // inv = ceil(2^20 / qw) (+1 at most if v_rcp_f32 is an ulp high), and idx * (inv - 2^20/qw) * qw < 2^20
      // (checked exhaustively on the CPU, including +-1 ulp of the reciprocal)
      const uint32_t inv = (uint32_t)ceilf(1048576.0f * __builtin_amdgcn_rcpf((float)max(qw, 1)));
      for (int idx = sub; __ballot(idx < npair); idx += 16) {
        if (MODE == 0) RTUF_LANES(kLaneQuarterTrip, idx < npair);
        if (idx < npair) {
          const int yy = (int)((uint32_t)__mul24(idx, (int)inv) >> 20);
          raster_pair<MODE, LOW>(keys, q, x_base, y_base, qx0 + idx - __mul24(yy, qw), qy0 + 2 * yy, qy1, kf);
        }
      }
    }
    }
  }
  // workgroup-cooperative: the parked triangles (those that cover a large part of the tile: walls, close
  // links), one at a time, the box's run of candidate pairs spread over all four waves.  ONE wave loads, unpacks
  // and classifies a batch of them (a lane each) and leaves the records and what the others need to know in LDS; the
  // other three waves wait at the barrier instead of repeating the same two hundred instructions (with ten wall
  // records in every tile of a 720p frame that repetition was 30 % of the walls' cost).
  __syncthreads();
  const uint32_t nh = min(s_huge[0], (uint32_t)kHugeMax);
  uint32_t zfull = zcover;                       // largest depth any pixel of the tile can still have (24-bit)
  for (uint32_t hb = 0; hb < nh; hb += 64) {
    const bool have = hb + (uint32_t)lane < nh;
    if (tid < 64) {
      TriRec r;
      if (have) {
        PackedTri pk;
        const uint4* src = reinterpret_cast<const uint4*>(recs + s_huge[1 + hb + lane]);
        uint4* dst = reinterpret_cast<uint4*>(&pk);
        dst[0] = src[0]; dst[1] = src[1];
        r = unpack_record(pk, width, height);
        r.order <<= kf.shift;
      } else {
#pragma unroll
        for (int k = 0; k < 16; k++) reinterpret_cast<int*>(&r)[k] = 0;
      }
      // per lane: the record's part of the tile, whether it is covered entirely, and the range of its depth
      // there.  The plane is evaluated exactly like fragment() does, which is monotonic in px and in py, so
      // the extremes over the box are at its corners.
      const int lx0 = max((int)(r.bbx & 0xffff) - x_base, 0), lx1 = min((int)(r.bbx >> 16) - x_base, kTileW - 1);
      const int ly0 = max((int)(r.bby & 0xffff) - y_base, 0), ly1 = min((int)(r.bby >> 16) - y_base, kTileH - 1);
      const int cls = have ? classify_box(r, x_base, y_base, lx0, lx1, ly0, ly1) : 0;
      const float cx0 = __fmaf_rn(r.dzdx, (float)(x_base + lx0), r.a0), cx1 = __fmaf_rn(r.dzdx, (float)(x_base + lx1), r.a0);
      const float fy0 = (float)(y_base + ly0), fy1 = (float)(y_base + ly1);
      const float z00 = __fmaf_rn(r.dzdy, fy0, cx0), z10 = __fmaf_rn(r.dzdy, fy0, cx1);
      const float z01 = __fmaf_rn(r.dzdy, fy1, cx0), z11 = __fmaf_rn(r.dzdy, fy1, cx1);
      const uint32_t zmin24 = z24_of(fminf(fminf(z00, z10), fminf(z01, z11))), zmax24 = z24_of(fmaxf(fmaxf(z00, z10), fmaxf(z01, z11)));
      const bool whole = cls == 2 && lx0 == 0 && ly0 == 0 && lx1 == min(kTileW, width - x_base) - 1 && ly1 == min(kTileH, height - y_base) - 1;
      if (have) {
        const uint4* sp = reinterpret_cast<const uint4*>(&r);
        uint4* dp = reinterpret_cast<uint4*>(&s_prec[lane]);
        dp[0] = sp[0]; dp[1] = sp[1]; dp[2] = sp[2]; dp[3] = sp[3];
        s_pmeta[lane] = make_uint4((uint32_t)cls, zmin24, whole ? zmax24 : 0xffffffffu, 0u);
      }
    }
    __syncthreads();
    uint4 meta = make_uint4(0u, 0xffffffffu, 0xffffffffu, 0u);
    if (have) meta = s_pmeta[lane];
    const uint32_t zmin24 = meta.y;
    // Occlusion among them: once a triangle covers every pixel of the tile, no pixel's key can have a
    // larger depth than that triangle's largest; a triangle whose smallest depth here is larger still
    // (the back of a wall, the wall behind it) cannot win anywhere in this tile and is skipped.
    uint32_t zf = meta.z;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) zf = min(zf, (uint32_t)__shfl_xor((int)zf, o));
    zfull = min(zfull, zf);
    unsigned long long m = __ballot(have && zmin24 <= zfull);
    const unsigned long long full = __ballot(have && meta.x == 2u);
    while (m) {
      const int src = __ffsll((long long)m) - 1;
      m &= m - 1;
      const bool inside = ((full >> src) & 1ull) != 0;
      TriRec q;                                        // the record from LDS into scalar registers (same address in every lane)
      {
        const uint4* sp = reinterpret_cast<const uint4*>(&s_prec[src]);
        uint4 w[4] = {sp[0], sp[1], sp[2], sp[3]};
        const int* wi = reinterpret_cast<const int*>(w);
        int* d = reinterpret_cast<int*>(&q);
#pragma unroll
        for (int k = 0; k < 16; k++) d[k] = __builtin_amdgcn_readfirstlane(wi[k]);
      }
      const int qx0 = max((int)(q.bbx & 0xffff) - x_base, 0), qx1 = min((int)(q.bbx >> 16) - x_base, kTileW - 1);
      const int qy0 = max((int)(q.bby & 0xffff) - y_base, 0), qy1 = min((int)(q.bby >> 16) - y_base, kTileH - 1);
      const int qw = qx1 - qx0 + 1, npair = qw * ((qy1 - qy0 + 2) >> 1);
      const uint32_t inv = (uint32_t)ceilf(1048576.0f * __builtin_amdgcn_rcpf((float)qw));
      if (inside && qw == kTileW) {
        // the triangle covers the tile's full width on these rows (the interior of a wall): one column per
        // lane, the waves interleave the rows; per pixel one fma on top of the column's part of the plane
        // (the same two roundings as fragment()), the 24-bit conversion and the LDS atomic
        const int px = x_base + lane;
        const float zc = __fmaf_rn(q.dzdx, (float)px, q.a0);
        for (int ly = qy0 + (tid >> 6); ly <= qy1; ly += NT / 64) {
          if (MODE == 0) { RTUF_LANES(kLaneParkTrip, true); RTUF_LANES(kLaneParkFrag, true); }
          const float z = __fmaf_rn(q.dzdy, (float)(y_base + ly), zc);
          const unsigned long long key = ((unsigned long long)((!LOW && MODE == 0) ? z24_of_upper_half(z) : z24_of(z)) << 32) | (LOW ? (q.order | (__float_as_uint(z) & kf.lowmask)) : q.order);
          const int lidx = ly * kKeyStride + lane;
          if (MODE == 0) {
            RTUF_COUNT_TEST();
            atomicMin(&keys[lidx], key);
          } else {
            if (keys[lidx] == key) keys[lidx] = resolved_key(key, z, kf);
          }
        }
      } else if (inside) {
        for (int idx = tid; idx < npair; idx += NT) {
          if (MODE == 0) RTUF_LANES(kLaneParkTrip, true);
          const int yy = (int)((uint32_t)__mul24(idx, (int)inv) >> 20);
          const int lx = qx0 + idx - __mul24(yy, qw), ly = qy0 + 2 * yy;
          const int lidx = ly * kKeyStride + lx;
          fragment<MODE, LOW>(keys, q, x_base + lx, y_base + ly, lidx, kf, kLaneParkFrag);
          if (ly < qy1) fragment<MODE, LOW>(keys, q, x_base + lx, y_base + ly + 1, lidx + kKeyStride, kf, kLaneParkFrag);
        }
      } else {
        for (int idx = tid; idx < npair; idx += NT) {
          if (MODE == 0) RTUF_LANES(kLaneParkTrip, true);
          const int yy = (int)((uint32_t)__mul24(idx, (int)inv) >> 20);
          raster_pair<MODE, LOW>(keys, q, x_base, y_base, qx0 + idx - __mul24(yy, qw), qy0 + 2 * yy, qy1, kf, kLaneParkFrag);
        }
      }
    }
    if (hb + 64 < nh) __syncthreads();               // (more than 64 parked: the next batch overwrites the LDS records)
  }
}

#ifndef RTUF_FRAG_UNROLL
#define RTUF_FRAG_UNROLL 4
#endif
constexpr int kFragUnroll = RTUF_FRAG_UNROLL;
// Fragments of the small triangles: 8 bytes each, perfectly coalesced, one LDS atomic each.  They never need the exact-float-z
// pass (the set-up kernel keeps anything with window z near 0.5 or below as a record).  kFragUnroll fragments per lane and
// trip, ALL their loads issued before the first is used: the loop used to be load -> wait -> one LDS atomic, one exposed
// global-memory latency per 256 fragments of a tile (a tile of the headline workload holds ~1,000): tile kernel 297 -> 285 us.
// The first trip's loads are issued by the caller before the key tile is initialised (load_frags / apply_frags).
template <int NT>
__device__ __forceinline__ void load_frags(unsigned long long (&f)[kFragUnroll], const unsigned long long* frags, uint32_t nf, uint32_t base, int tid)
{
#pragma unroll
  for (int u = 0; u < kFragUnroll; u++) {
    const uint32_t i = base + (uint32_t)u * NT + (uint32_t)tid;
    f[u] = i < nf ? frags[i] : ~0ull;
  }
}
template <int NT>
__device__ __forceinline__ void apply_frags(unsigned long long* keys, const unsigned long long (&f)[kFragUnroll], uint32_t nf, uint32_t base, int tid, uint32_t zcover, int shift)
{
#pragma unroll
  for (int u = 0; u < kFragUnroll; u++) {
    const uint32_t i = base + (uint32_t)u * NT + (uint32_t)tid;
    const int fpos = (int)((uint32_t)f[u] & ((1u << kFragPosBits) - 1u));      // row * kTileW + column: the key's index
    const unsigned long long key = ((f[u] >> 40) << 32) | (((uint32_t)(f[u] >> kFragPosBits) & kMaxOrder) << shift);
    // (zcover == 0xffffffff: no cover, every fragment passes; behind the tile's cover: cannot win)
    RTUF_LANES(kLaneFragList, i < nf && (uint32_t)(f[u] >> 40) <= zcover);
    if (i < nf && (uint32_t)(f[u] >> 40) <= zcover) { RTUF_COUNT_TEST(); atomicMin(&keys[fpos], key); }
  }
}

// The output planes (and, in the compare kernel, the sensor plane) are touched exactly once: non-temporal
// accesses keep them from displacing the bins and the geometry in L2 / MALL (tile kernel -3 %, compare
// kernel -6 %).
__device__ __forceinline__ void store_stream4(float* dst, float a, float b, float c, float d)
{
  __builtin_nontemporal_store(a, dst); __builtin_nontemporal_store(b, dst + 1);
  __builtin_nontemporal_store(c, dst + 2); __builtin_nontemporal_store(d, dst + 3);
}
__device__ __forceinline__ void store_stream4(uint16_t* dst, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
  uint32_t* w = reinterpret_cast<uint32_t*>(dst);
  __builtin_nontemporal_store(a | (b << 16), w); __builtin_nontemporal_store(c | (d << 16), w + 1);
}
// four link labels (two per word) as one 8-byte non-temporal store
__device__ __forceinline__ void store_labels4(uint16_t* dst, uint32_t lo, uint32_t hi)
{
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  u32x2 v;
  v.x = lo; v.y = hi;
  __builtin_nontemporal_store(v, reinterpret_cast<u32x2*>(dst));
}
__device__ __forceinline__ float4 load_stream4(const float* src)
{
  return make_float4(__builtin_nontemporal_load(src), __builtin_nontemporal_load(src + 1),
                     __builtin_nontemporal_load(src + 2), __builtin_nontemporal_load(src + 3));
}

// 16UC1 <-> float exactly like the reference's cv::Mat::convertTo calls:
//   in : convertTo(CV_32F, 0.001)  -> float(u16) * 0.001f               (src/urdf_filter.cpp:287-288)
//   out: convertTo(CV_16U, 1000.0) -> saturate_cast<ushort>(cvRound(v * 1000.0f)): round half to even,
//        NaN / out-of-int-range -> "integer indefinite" -> 0, otherwise clamped to [0, 65535]   (:309-312)
__device__ __forceinline__ float u16_to_metres(uint32_t u) { return __fmul_rn((float)u, 0.001f); }
__device__ __forceinline__ uint32_t metres_to_u16(float m)
{
  const float v = __fmul_rn(m, 1000.0f);
  if (!(v >= -2147483648.0f && v < 2147483648.0f)) return 0u;
  const int i = __float2int_rn(v);
  return (uint32_t)min(max(i, 0), 65535);
}

// urdf_filter.frag:14-35.  num = z_near*z_far/(z_near-z_far), off = z_far/(z_far-z_near): evaluated once per batch on the
// host, in float, exactly as the shader's to_linear_depth does (shade_num / shade_off, rtuf_numerics.h).  core: the host
// admits div_core for the two constants (fast_div_admitted).
struct ShadeConsts { float num, off, max_diff, replace_value; bool core; };

// sensor > shade_threshold(z)  <=>  should_filter of include/shaders/urdf_filter.frag:22-23
__device__ __forceinline__ float shade_threshold(float z, const ShadeConsts& k)
{
  const float d = __fsub_rn(z, k.off);
  const float virt = k.core ? div_core(k.num, d) : __fdiv_rn(k.num, d);
  return __fsub_rn(virt, k.max_diff);
}
// the virtual depth itself, to_linear_depth(gl_FragCoord.z): shade_threshold without its subtraction (rtuf_render_batch*)
__device__ __forceinline__ float shade_virtual(float z, const ShadeConsts& k)
{
  const float d = __fsub_rn(z, k.off);
  return k.core ? div_core(k.num, d) : __fdiv_rn(k.num, d);
}
// the same with a threshold of its own in place of max_diff (per-link depth thresholds)
__device__ __forceinline__ float shade_threshold(float z, const ShadeConsts& k, float max_diff)
{
  const float d = __fsub_rn(z, k.off);
  const float virt = k.core ? div_core(k.num, d) : __fdiv_rn(k.num, d);
  return __fsub_rn(virt, max_diff);
}

__device__ __forceinline__ float shade(float sensor, float z, const ShadeConsts& k, bool& filt)
{
  filt = sensor > shade_threshold(z, k);
  return filt ? k.replace_value : sensor;
}

// Link residual tables (rtuf_link_residuals_batch*): the reduction of a resolve pass.  Every lane brings four pixels' class
// bits (rtuf_numerics.h, 0: outside the image), labels and quantised residuals.  While pixels remain, the wave takes the first
// remaining pixel's label, ballots the pixels that share it, popcounts the six class ballots, wave-sums q and |q| of the
// agree pixels among them, and eight lanes add the row's eight 64-bit values (zero addends skipped) -- not to the table but to
// the workgroup's copy of the row in LDS: kResidSlots rows in the exact-z pass's record buffer, dead at resolve time, found by
// linear probing over their label tags; the workgroup's last step adds every used row to the table, one 64-byte line per
// label.  All waves of a stream's tiles add to the same few rows, and adders of one line are served one after the other; with
// this a tile has one per (label, field) instead of one per wave and pass (reasoned, not measured against the direct form).  A workgroup that sees more than kResidSlots labels adds the surplus to the table directly.
constexpr int kResidSlots = 16;
constexpr uint32_t kResidFree = 0xffffffffu;      // (labels are 16 bits wide)
__device__ __forceinline__ void resid_reduce(const uint32_t (&cls)[4], const uint32_t (&lab)[4], const int (&q)[4], unsigned long long* rows, uint32_t* tags,
                                             unsigned long long* table_rows)
{
  const int lane = (int)(threadIdx.x & 63u);
  uint32_t rem = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) rem |= (cls[j] & kResPixel) << j;
  for (;;) {
    const unsigned long long live = __ballot(rem != 0u);
    if (!live) break;
    uint32_t mine = 0u;                      // the label of the lane's first remaining pixel
#pragma unroll
    for (int j = 3; j >= 0; j--) mine = (rem >> j & 1u) != 0u ? lab[j] : mine;
    const uint32_t label = (uint32_t)__builtin_amdgcn_readlane((int)mine, __ffsll((long long)live) - 1);
    uint32_t cnt[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    long long sq = 0;
    unsigned long long sa = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const bool in = (rem >> j & 1u) != 0u && lab[j] == label;
      const uint32_t c = in ? cls[j] : 0u;
      if (in) rem &= ~(1u << j);
#pragma unroll
      for (int f = 0; f < 6; f++) cnt[f] += (uint32_t)__popcll(__ballot((c >> f & 1u) != 0u));
      if (c & kResAgree) { sq += (long long)q[j]; sa += (unsigned long long)(q[j] < 0 ? -(long long)q[j] : (long long)q[j]); }
    }
    if (cnt[5]) {                            // (uniform) sums over the wave: in 32 bits where 64 lanes' sums cannot leave them
      if (__ballot(sa >= (1ull << 25)) == 0ull) {
        int s32 = (int)sq, a32 = (int)sa;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { s32 += __shfl_xor(s32, d); a32 += __shfl_xor(a32, d); }
        sq = (long long)s32; sa = (unsigned long long)(uint32_t)a32;
      } else {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { sq += __shfl_xor(sq, d); sa += __shfl_xor(sa, d); }
      }
    }
    // the row's slot in LDS: the first free or equal tag from the label's home on (-1: every slot holds another label)
    int slot = -1;
    for (int i = 0; i < kResidSlots && slot < 0; i++) {
      const int idx = (int)((label + (uint32_t)i) & (uint32_t)(kResidSlots - 1));
      uint32_t old = 0u;
      if (lane == 0) old = atomicCAS(&tags[idx], kResidFree, label);
      old = (uint32_t)__builtin_amdgcn_readfirstlane((int)old);
      if (old == kResidFree || old == label) slot = idx;
    }
    unsigned long long val = (unsigned long long)cnt[0];
#pragma unroll
    for (int f = 1; f < 6; f++) val = lane == f ? (unsigned long long)cnt[f] : val;
    val = lane == 6 ? (unsigned long long)sq : val;
    val = lane == 7 ? sa : val;
    if (lane < 8 && val != 0ull) {
      if (slot >= 0) atomicAdd(&rows[slot * 8 + lane], val);
      else atomicAdd(&table_rows[(size_t)label * 8u + (uint32_t)lane], val);
    }
  }
}

// COVER: the batch ran the cover pass (bigrec_kernel<0>), so a bin's header may name a cover.  Without it (the host skips the
// pass while no scene has triangles that cover whole tiles) the cover code is compiled out: it costs the headline workload 3 %.
// LABELS: the kernel also writes the link label plane (a.labels, a.order_labels: rtuf_filter_batch*_labels).
// THRESH: a drawn pixel is compared with its winner's link threshold (a.order_thr: rtuf_set_link_thresholds) instead of
// max_diff; the background plane keeps thr_bg.
// OUT (rtuf_routes.h, where tile_variant_legal says which of LABELS and THRESH each output may carry):
// Planes: the masked plane and the byte mask, compared here.  ZSurface (TWO_KERNEL below): the winners' window z for the
// kernel behind this one.  Bits: the mask only, one bit per pixel.
// Render: no sensor plane, no compare: the only outputs are the virtual depth plane (a.virtual_out: shade_virtual of every
// winner's z, a.empty_value where the background quad won or nothing was drawn; U16: both through metres_to_u16) and, with
// LABELS, the label plane (rtuf_render_batch*).
// Residual (RESID below): no output plane at all: every pixel of the image is classified against the sensor plane
// (link_residual_class: virtual depth, the winner's threshold -- a.order_thr's with THRESH, max_diff without -- and label) and
// counted in its label's row of the stream's table (a.resid_table: rtuf_link_residuals_batch*; resid_reduce).
template <TileOut OUT, bool U16, bool COVER, int NT, bool LABELS = false, bool THRESH = false>
__device__ __forceinline__ void tile_body(const TileArgs& a)
{
  static_assert(tile_variant_legal(TileVariant{OUT, LABELS, THRESH, U16, COVER}), "no such variant of the tile kernel (rtuf_routes.h)");
  constexpr bool TWO_KERNEL = OUT == TileOut::ZSurface, BITS = OUT == TileOut::Bits, RENDER = OUT == TileOut::Render, RESID = OUT == TileOut::Residual;
  __shared__ unsigned long long keys[kKeyCount];
  __shared__ uint32_t s_huge[2 + kHugeMax];        // raster_bin's list of whole-tile triangles (+ count in front, area threshold behind)
  __shared__ uint32_t s_winners[kWinnerWords];     // exact-z pass: filter of the draw-order keys that won a pixel in need
  __shared__ TriRec s_prec[64];                    // ... a batch of them unpacked by the first wave for all four,
  __shared__ uint4 s_pmeta[64];                    //     with {class, smallest depth, largest depth if it covers the whole tile}

  const int tid = threadIdx.x;
  RTUF_LANES_INIT(1);
  const int tiles = a.tiles_x * a.tiles_y;
  // grid = (tiles_x, tiles_y, streams of the group): no integer divisions to find the tile
  const int txi = blockIdx.x, tyi = blockIdx.y, slot = blockIdx.z;
  const int bin = slot * tiles + tyi * a.tiles_x + txi;
  const int stream = a.group_base + slot;
  const int x_base = txi * kTileW, y_base = tyi * kTileH;

  // the record bin's two fill counters and the tile's cover (the nearest triangle that covers this whole tile, if any:
  // bound of every key's depth, and its plane) in ONE 16-byte scalar load, the fragment bin's counter in a second one
  uint32_t count_front, count_back;
  unsigned long long cover;
  {
    const uint4 h = *reinterpret_cast<const uint4*>(a.bin_hdr + bin);
    count_front = h.x; count_back = h.y;
    cover = COVER ? ((unsigned long long)h.w << 32) | h.z : kNoCover;
  }
  // fragment count, and in the top bit: the bin holds a near record (or its cover is one): the depth keys of this tile
  // carry the low bits of the float z (KeyFmt)
  const uint32_t fraw = a.fbin_count[bin];
  const uint32_t fcount = fraw & 0x7fffffffu;
  const bool near_tile = (fraw >> 31) != 0u;              // (wave-uniform: a scalar load of a workgroup-uniform address)
  KeyFmt kf;
  kf.shift = a.key_shift;
  kf.abl = a.flags;
  kf.lowmask = near_tile ? (1u << a.key_shift) - 1u : 0u;
  kf.zexact = near_tile ? exact_z_floor(a.key_shift) : 8388609u;
  kf.keep_order = LABELS || THRESH || RENDER || RESID;      // (RENDER: order 0 is the background quad drawn as geometry)
  const uint32_t count = count_front + count_back;
  // (the stream's background entry after the bin's header in program order: the compiler then issues the three scalar loads
  // together -- with the background first it waited for it before it even computed the header's address)
  const BgInfo bi = a.bg[stream];
  const bool analytic_bg = bi.mode != 0;
  const float bgz = bi.z, thr_bg = bi.thr;
  const unsigned long long bgkey = analytic_bg ? ((unsigned long long)bi.z24 << 32) : kNoFragment;
  ShadeConsts sc;
  sc.num = a.sc_num; sc.off = a.sc_off; sc.max_diff = a.max_diff; sc.replace_value = a.replace_value; sc.core = a.fast_div != 0;
  const uint32_t zcover = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(cover >> 32));      // (<= 0xffffff, or all ones: none)
  const uint32_t cover_idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)cover);
  const bool has_cover = zcover != 0xffffffffu;
  // The sensor pixels this lane will resolve.  A tile without geometry requests them as soon as the bin header says so (that
  // latency is all there is to such a tile); a tile with geometry requests them after the rasterisation: eight registers
  // held across the walks do not fit the kernel's 80-register budget (they spill, and the spill waits for the load), and
  // requesting them early AND late costs more in traffic than the early request hides (both measured, profiles/README.md).
  constexpr int kLanesPerRow = kTileW / 4, kRowsPerPass = NT / kLanesPerRow;
  constexpr int kPasses = (kTileH + kRowsPerPass - 1) / kRowsPerPass;      // resolve passes per tile (2 for 64x32)
  const bool vec = (a.width & 3) == 0;
  const int r_ly0 = tid / kLanesPerRow, r_lx = (tid % kLanesPerRow) * 4;
  const int r_px = x_base + r_lx;
  float4 sens_p[kPasses];
  auto request_sensor = [&]() {
#pragma unroll
    for (int ps = 0; ps < kPasses; ps++) {
      const int r_ly = r_ly0 + ps * kRowsPerPass, r_py = y_base + r_ly;
      const bool r_valid = r_ly < kTileH && r_py < a.height && r_px < a.width;
      // 64-bit part uniform (scalar), per-lane part 24-bit (W, H <= 2048)
      const size_t gofs = (size_t)stream * ((size_t)a.height * a.width) + (uint32_t)(__mul24(r_py, a.width) + r_px);
      sens_p[ps] = make_float4(0, 0, 0, 0);
      if (!TWO_KERNEL && r_valid && vec) {
        if (U16) {
          const ushort4 q = *reinterpret_cast<const ushort4*>(reinterpret_cast<const uint16_t*>(a.depth) + gofs);
          sens_p[ps] = make_float4(u16_to_metres(q.x), u16_to_metres(q.y), u16_to_metres(q.z), u16_to_metres(q.w));
        } else {
          sens_p[ps] = *reinterpret_cast<const float4*>(a.depth + gofs);
        }
      }
    }
  };
  // (an over-full bin is detected from the counters and the batch run again; until then stay inside the array)
  const uint32_t n_front = min(count_front, a.capacity), n = n_front + min(count_back, a.capacity - n_front), nf = min(fcount, a.fcapacity);
  const PackedTri* recs = a.bins + (size_t)bin * a.capacity;
  const unsigned long long* frags = reinterpret_cast<const unsigned long long*>(a.fbins) + (size_t)bin * a.fcapacity;
  // (RTUF_ABLATE builds only: flags bits 8.. are timing experiments, e.g. 0x100 skip rasterisation, 0x200 skip pixel loops)
  const bool empty = (n == 0 && nf == 0 && !has_cover) || RTUF_ABL(a.flags, 0x100u);   // no geometry in this tile: pure streaming compare
  if (empty && RTUF_ABL(a.flags, 0x1000000u)) return;               // timing experiment: raster tiles only
  // A tile that a triangle covers entirely and that holds NOTHING else (the wall behind the robot, wherever the robot is not:
  // most tiles of BASELINE config 4) needs no key tile either: every pixel is the cover's fragment or the background's,
  // decided and shaded from registers -- the same two fused multiply-adds, 24-bit conversion and key comparison the key tile
  // would see, and the fragment's float z at hand instead of rebuilt from the key.  One barrier (before the bin header is reset
  // for the next batch: every wave must have read it) instead of three, no LDS traffic.  Only in the kernels that run with the
  // cover pass: the others' code is what it was (this kernel sits on its register budget: a variable more in scope of the
  // common path cost the headline workload 20 % when this was first written for all variants).
  bool cover_only = false;
  float cov_a0 = 0.0f, cov_dzdx = 0.0f, cov_dzdy = 0.0f;
  uint32_t cov_label = 0;                    // LABELS: the cover's link label, one lookup per tile
  float cov_thr = 0.0f;                      // THRESH: the cover's link threshold, one lookup per tile
  bool cov_robot = true;                     // RENDER: the cover is a link's triangle, not the background quad drawn as geometry
  // the cover's z plane and draw order, from the record the bin's header points to
  struct CoverPlane { float a0, dzdx, dzdy; uint32_t order; };
  auto cover_plane = [&]() {
    const uint4 pl = reinterpret_cast<const uint4*>(a.big_list + cover_idx)[1];       // {a0, dzdx, dzdy, order}: same address in every lane
    CoverPlane c;
    c.a0 = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)pl.x));
    c.dzdx = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)pl.y));
    c.dzdy = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)pl.z));
    c.order = (uint32_t)__builtin_amdgcn_readfirstlane((int)pl.w) & kOrderMask;
    return c;
  };
  if constexpr (COVER) {
    cover_only = has_cover && n == 0 && nf == 0 && !empty;
    if (cover_only) {
      if (!RENDER) request_sensor();
      const CoverPlane c = cover_plane();
      cov_a0 = c.a0; cov_dzdx = c.dzdx; cov_dzdy = c.dzdy;
      if (LABELS || RESID) cov_label = a.order_labels[c.order];
      if (THRESH) cov_thr = a.order_thr[c.order];
      if (RENDER) cov_robot = c.order != 0u;
#ifdef RTUF_COUNT
      if (tid < 2) count_words()[tid] = 0u;
#endif
      __syncthreads();
      if (tid == 0) {
        *reinterpret_cast<uint4*>(a.bin_hdr + bin) = make_uint4(0u, 0u, 0xffffffffu, 0xffffffffu);      // ready for the next batch: nothing binned, no cover
        a.fbin_count[bin] = 0;                                                                          // (a near cover had set the near flag)
        atomicAdd(&a.counters->shard[bin % kCounterShards].cover_tiles, 1u);
      }
    }
  }
  if (empty && !RENDER) request_sensor();
  if (!empty && !cover_only) {
    // Initial depth keys: the background plane and, where a triangle covers the whole tile, that triangle's fragments --
    // evaluated per pixel exactly as fragment() would (same two fused multiply-adds, same 24-bit conversion, its draw
    // order), but written instead of min'ed: it is the first thing the tile sees, and bigrec_kernel<1> left it out of the bin.
    // (the plane is fetched again by the rare exact-z pass below rather than kept in registers across the rasterisation)
    // Ask for the first things this lane will need from the bins BEFORE the key tile is initialised: its first record and
    // its first fragments (their latency then passes under the initialisation and the barrier instead of after it).
    uint4 first_rec0 = make_uint4(0u, 0u, 0u, 0u), first_rec1 = make_uint4(0u, 0u, 0u, 0u);
    if ((uint32_t)tid < n) {
      const uint4* src = reinterpret_cast<const uint4*>(recs + ((uint32_t)tid < n_front ? (uint32_t)tid : a.capacity - 1u - ((uint32_t)tid - n_front)));
      first_rec0 = src[0]; first_rec1 = src[1];
    }
    unsigned long long first_frags[kFragUnroll];
    load_frags<NT>(first_frags, frags, nf, 0u, tid);
    if (has_cover) {
      const CoverPlane c = cover_plane();
      for (int i = tid; i < kKeyCount; i += NT) {
        const float z = __fmaf_rn(c.dzdy, (float)(y_base + i / kKeyStride), __fmaf_rn(c.dzdx, (float)(x_base + i % kKeyStride), c.a0));
        const unsigned long long key = ((unsigned long long)z24_of(z) << 32) | (c.order << kf.shift) | (__float_as_uint(z) & kf.lowmask);
        keys[i] = min(key, bgkey);
      }
    } else {
      for (int i = tid; i < kKeyCount; i += NT) keys[i] = bgkey;
    }
    if (tid == 0) { s_huge[0] = 0; s_huge[1 + kHugeMax] = n <= (uint32_t)kParkBelow ? (uint32_t)kQuarterArea : (uint32_t)kWallArea; }
#ifdef RTUF_COUNT
    if (tid < 2) count_words()[tid] = 0u;
#endif
    __syncthreads();
    if (tid == 0) {
      *reinterpret_cast<uint4*>(a.bin_hdr + bin) = make_uint4(0u, 0u, 0xffffffffu, 0xffffffffu);      // ready for the next batch: nothing binned, no cover
      a.fbin_count[bin] = 0;
      CounterShard& sh = a.counters->shard[bin % kCounterShards];
      if (count) atomicMax(&sh.max_bin_fill, count);
      if (fcount) atomicMax(&sh.max_fbin_fill, fcount);
      if (has_cover) atomicAdd(&sh.cover_tiles, 1u);
#ifdef RTUF_HIST            // (scripts/bin_hist.sh, never the product: how much of the bins lies beyond a direct capacity of RTUF_HIST)
      {
        const uint32_t cls_count = RTUF_HIST_BACK ? count_back : count_front;
        if (cls_count > (uint32_t)RTUF_HIST) atomicAdd(&sh.raster_atomics, (1ull << 40) + (cls_count - (uint32_t)RTUF_HIST));
        if (fcount > 4u * RTUF_HIST) atomicAdd(&sh.drawn_pixels, (1ull << 40) + (fcount - 4u * RTUF_HIST));
      }
#endif
    }
    // fragments first (one LDS atomic each; the first trip's are in registers already), then the records
    // (two instances of the rasterisation: tiles without near geometry -- every tile of a robot at arm's length -- do not
    // pay the instruction that puts the float's low bits into the key)
    {
      bool do_frags = true, do_records = true, load_only = false;
      int skip = 0;
#ifdef RTUF_ABLATE
      do_frags = !(a.flags & 0x400u); do_records = !(a.flags & 0x800u); load_only = (a.flags & 0x200u) != 0; skip = (int)((a.flags >> 12) & 3u);
#endif
      if (do_frags) {
        apply_frags<NT>(keys, first_frags, nf, 0u, tid, zcover, kf.shift);
        for (uint32_t base = kFragUnroll * NT; base < nf; base += kFragUnroll * NT) {
          unsigned long long f[kFragUnroll];
          load_frags<NT>(f, frags, nf, base, tid);
          apply_frags<NT>(keys, f, nf, base, tid, zcover, kf.shift);
        }
      }
      if (do_records) {
        if (near_tile) raster_bin<0, true, NT>(keys, recs, n, x_base, y_base, tid, load_only, a.width, a.height, n_front, a.capacity, s_huge, s_prec, s_pmeta, zcover, s_winners, kf, first_rec0, first_rec1, true, skip);
        else raster_bin<0, false, NT>(keys, recs, n, x_base, y_base, tid, load_only, a.width, a.height, n_front, a.capacity, s_huge, s_prec, s_pmeta, zcover, s_winners, kf, first_rec0, first_rec1, true, skip);
      }
    }
    __syncthreads();
    if (tid == 0) s_huge[0] = 0;             // the exact-z pass below builds its list again

    // Does any pixel need a second look for the exact float z of its winner?  In the upper half of the depth range
    // (z24 > 2^23) float z == (z24 + 1) * 2^-24 exactly; below, a tile with near geometry has the float's low bits in its
    // keys, which settle everything but the last micrometres in front of the near plane (z24 < zexact); a tile without
    // them has no record that could get there at all (the set-up marks those near) -- the test stays, it costs nothing.
    // (round 6: a tile without near geometry does not look -- no record, fragment or cover of it can produce z < 0.51, which is
    // what its depth tests already rely on (z24_of_upper_half) -- and is spared eight key reads per lane and a barrier)
    bool need = false;
    if (near_tile) {
      for (int i = tid; i < kKeyCount; i += NT) {
        const unsigned long long k = keys[i];
        if (k != bgkey && (uint32_t)(k >> 32) < kf.zexact) need = true;
      }
      need = __syncthreads_or(need) != 0;
    }
    if (need && !RTUF_ABL(a.flags, 0x4000000u)) {      // (0x4000000: timing experiment, no exact-z pass)
      // which draw-order keys won such a pixel: only their records are walked again
      if (tid < kWinnerWords) s_winners[tid] = 0u;
      if (tid == 0) atomicAdd(&a.counters->shard[bin % kCounterShards].exact_tiles, 1u);
      __syncthreads();
      for (int i = tid; i < kKeyCount; i += NT) {
        const unsigned long long k = keys[i];
        if (k != bgkey && (uint32_t)(k >> 32) < kf.zexact) {
          const uint32_t h = winner_slot((uint32_t)k >> kf.shift);
          atomicOr(&s_winners[h >> 5], 1u << (h & 31u));
        }
      }
      __syncthreads();
      raster_bin<1, true, NT>(keys, recs, n, x_base, y_base, tid, false, a.width, a.height, n_front, a.capacity, s_huge, s_prec, s_pmeta, zcover, s_winners, kf, first_rec0, first_rec1, false);
      if (has_cover) {                       // ... and the cover triangle, which is in no bin
        const CoverPlane c = cover_plane();
        for (int i = tid; i < kKeyCount; i += NT) {
          const float z = __fmaf_rn(c.dzdy, (float)(y_base + i / kKeyStride), __fmaf_rn(c.dzdx, (float)(x_base + i % kKeyStride), c.a0));
          const unsigned long long key = ((unsigned long long)z24_of(z) << 32) | (c.order << kf.shift) | (__float_as_uint(z) & kf.lowmask);
          if (keys[i] == key) keys[i] = resolved_key(key, z, kf);
        }
      }
      __syncthreads();
    }
    // (requested here, not before the scan above: with the eight registers live from there the kernel sits at its 80-register
    // limit and the allocation of everything before it suffers -- measured once more in round 4: tile kernel 296 instead of 280 us)
    if (!RENDER) request_sensor();
  }

  // resolve: kLanesPerRow lanes x 4 pixels per tile row, kRowsPerPass rows per pass.  `finish` turns four
  // window depths (or "nothing drawn") and their compare thresholds into the outputs.
  // With BITS the only output is one mask bit per pixel: `finish` returns the lane's four mask flags (bit j = pixel j)
  // and stores nothing; the caller packs the flags of 8 neighbouring lanes into one 32-bit word.
  bool uncovered = false;                              // BITS: a pixel no fragment reached (its masked depth would be the clear colour, not the sensor value)
  // RESID: the workgroup's table rows and their label tags in LDS the rasterisation is done with (every use of it above ends
  // at a barrier), and what `finish` leaves of a pass for resid_reduce: class bits, label and quantised residual per pixel.
  // In this mode `finish` takes the virtual depths for z and the thresholds themselves (t, not virtual - t) for thr; the
  // background plane's virtual depth is the division the pose kernel's thr_bg holds (IEEE, as BgInfo::thr).
  unsigned long long* const rs_rows = reinterpret_cast<unsigned long long*>(s_prec);
  uint32_t* const rs_tags = s_winners;
  static_assert(!RESID || (sizeof(TriRec) * 64 >= sizeof(unsigned long long) * 8 * kResidSlots && kWinnerWords >= kResidSlots), "the residual rows live in s_prec / s_winners");
  uint32_t rs_cls[4] = {0u, 0u, 0u, 0u}, rs_lab[4] = {0u, 0u, 0u, 0u};
  int rs_q[4] = {0, 0, 0, 0};
  float rs_vbg = 0.0f;
  if (RESID) {
    rs_vbg = __fdiv_rn(a.sc_num, __fsub_rn(bgz, a.sc_off));
    if (tid < kResidSlots * 8) rs_rows[tid] = 0ull;
    if (tid < kResidSlots) rs_tags[tid] = kResidFree;
    __syncthreads();
  }
  // LABELS: lab = the four pixels' link labels, stored to the stream's label plane in either route
  auto finish = [&](int ps, const float (&z)[4], const float (&thr)[4], const bool (&frag)[4], const uint32_t (&lab)[4]) -> uint32_t {
    const int r_ly = r_ly0 + ps * kRowsPerPass, py = y_base + r_ly, px = r_px;
    const size_t gofs = (size_t)stream * ((size_t)a.height * a.width) + (uint32_t)(__mul24(py, a.width) + px);
    const int nvalid = min(4, a.width - px);
    if (LABELS) {
      if (vec) store_labels4(a.labels + gofs, lab[0] | (lab[1] << 16), lab[2] | (lab[3] << 16));
      else for (int j = 0; j < nvalid; j++) a.labels[gofs + j] = (uint16_t)lab[j];
    }
    if (RENDER) {                            // z = the four virtual depths (or the empty value): the plane's only store
      if (vec) {
        if (U16) store_stream4(reinterpret_cast<uint16_t*>(a.virtual_out) + gofs, metres_to_u16(z[0]), metres_to_u16(z[1]), metres_to_u16(z[2]), metres_to_u16(z[3]));
        else store_stream4(a.virtual_out + gofs, z[0], z[1], z[2], z[3]);
      } else {
        for (int j = 0; j < nvalid; j++) {
          if (U16) reinterpret_cast<uint16_t*>(a.virtual_out)[gofs + j] = (uint16_t)metres_to_u16(z[j]);
          else a.virtual_out[gofs + j] = z[j];
        }
      }
      return 0u;
    }
    if (TWO_KERNEL) {
      const size_t zofs = (size_t)slot * ((size_t)a.height * a.width) + (uint32_t)(__mul24(py, a.width) + px);
      // "no fragment" (only without background quad) is encoded as NaN
      float zz[4];
#pragma unroll
      for (int j = 0; j < 4; j++) zz[j] = frag[j] ? z[j] : __uint_as_float(0x7fc00000u);
      if (vec) *reinterpret_cast<float4*>(a.zsurface + zofs) = make_float4(zz[0], zz[1], zz[2], zz[3]);
      else for (int j = 0; j < nvalid; j++) a.zsurface[zofs + j] = zz[j];
      return 0u;
    }
    float s[4];
    if (vec) {
      s[0] = sens_p[ps].x; s[1] = sens_p[ps].y; s[2] = sens_p[ps].z; s[3] = sens_p[ps].w;
    } else {
      for (int j = 0; j < 4; j++)
        s[j] = j < nvalid ? (U16 ? u16_to_metres(reinterpret_cast<const uint16_t*>(a.depth)[gofs + j]) : a.depth[gofs + j]) : 0.0f;
    }
    if (RESID) {                             // z = the virtual depths, thr = the thresholds: classes for resid_reduce, no store
#pragma unroll
      for (int j = 0; j < 4; j++) {
        int q = 0;
        uint32_t c = frag[j] ? link_residual_class(s[j], z[j], thr[j], q) : link_residual_undrawn(s[j]);
        if (j >= nvalid) c = 0u;
        rs_cls[j] = c; rs_lab[j] = lab[j]; rs_q[j] = q;
      }
      return 0u;
    }
    float o[4];
    uint32_t mbits = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      bool f = s[j] > thr[j];
      o[j] = f ? sc.replace_value : s[j];
      if (!frag[j]) { o[j] = 0.0f; f = false; if (BITS) uncovered = true; }     // GL clear colour
      if (f) mbits |= (BITS ? 1u : 0xffu) << ((BITS ? 1 : 8) * j);
    }
    if (BITS) return mbits;
    if (vec) {
      if (U16) {
        store_stream4(reinterpret_cast<uint16_t*>(a.masked) + gofs, metres_to_u16(o[0]), metres_to_u16(o[1]), metres_to_u16(o[2]), metres_to_u16(o[3]));
      } else {
        store_stream4(a.masked + gofs, o[0], o[1], o[2], o[3]);
      }
      if (a.mask) __builtin_nontemporal_store(mbits, reinterpret_cast<uint32_t*>(a.mask + gofs));
    } else {
      for (int j = 0; j < nvalid; j++) {
        if (U16) reinterpret_cast<uint16_t*>(a.masked)[gofs + j] = (uint16_t)metres_to_u16(o[j]);
        else a.masked[gofs + j] = o[j];
        if (a.mask) a.mask[gofs + j] = (uint8_t)(mbits >> (8 * j));
      }
    }
    return mbits;
  };
  // Most pixels of a frame see only the background plane, whose depth is one value per stream: its compare
  // threshold (one IEEE division) is computed once per lane.  Same operations on the same values as per pixel.
  const float bg_z4[4] = {bgz, bgz, bgz, bgz}, bg_thr4[4] = {thr_bg, thr_bg, thr_bg, thr_bg};
  const bool bg_frag4[4] = {analytic_bg, analytic_bg, analytic_bg, analytic_bg};
  const uint32_t no_lab4[4] = {0u, 0u, 0u, 0u};
  const float empty4[4] = {a.empty_value, a.empty_value, a.empty_value, a.empty_value};      // RENDER
  const float rs_vbg4[4] = {rs_vbg, rs_vbg, rs_vbg, rs_vbg}, rs_t4[4] = {a.max_diff, a.max_diff, a.max_diff, a.max_diff};      // RESID
#pragma unroll
  for (int ps = 0; ps < kPasses; ps++) {
    const int r_ly = r_ly0 + ps * kRowsPerPass;
    const bool valid = r_ly < kTileH && y_base + r_ly < a.height && r_px < a.width;
    uint32_t flags4 = 0;
    RTUF_LANES(kLaneResolve, valid);
    if (RESID) { rs_cls[0] = rs_cls[1] = rs_cls[2] = rs_cls[3] = 0u; }      // (lanes outside the image bring nothing)
    if (valid) {
      if (RESID && empty) {                          // tile without geometry: the background plane (or nothing drawn) in every pixel
        flags4 = finish(ps, rs_vbg4, rs_t4, bg_frag4, no_lab4);
      } else if (RENDER && empty) {                         // tile without geometry: a streaming store of the empty value
        flags4 = finish(ps, empty4, bg_thr4, bg_frag4, no_lab4);
      } else if (empty) {                            // tile without geometry: a streaming compare against the plane
        if (analytic_bg) {          // (uniform: with the flags known to be set the four selects on them fall away)
          const bool all4[4] = {true, true, true, true};
          flags4 = finish(ps, bg_z4, bg_thr4, all4, no_lab4);
        } else {
          flags4 = finish(ps, bg_z4, bg_thr4, bg_frag4, no_lab4);
        }
      } else if (COVER && cover_only) {      // nothing but a triangle over the whole tile: its fragment or the background's, from registers
        float z[4], thr[4];
        bool frag[4];
        uint32_t lab[4];
        const float zrow = (float)(y_base + r_ly);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float zf = __fmaf_rn(cov_dzdy, zrow, __fmaf_rn(cov_dzdx, (float)(r_px + j), cov_a0));
          // what atomicMin on a key tile initialised with the background would keep: the cover's key {z24, order << shift | low
          // bits} against the background's (or "no fragment"'s) {z24, 0} -- its draw order is at least 1, so it is below exactly
          // when its 24-bit depth is: one 32-bit compare, no key to put together; without near geometry (a near cover marks its
          // tile) the depth comes from the product's bit pattern like everywhere else
          const uint32_t cz24 = near_tile ? z24_of(zf) : z24_of_upper_half(zf);
          const bool drawn = cz24 < (uint32_t)(bgkey >> 32);
          z[j] = drawn ? zf : bgz;
          frag[j] = drawn ? true : analytic_bg;
          thr[j] = thr_bg;
          lab[j] = drawn ? cov_label : 0u;
          if (RENDER) z[j] = drawn && cov_robot ? shade_virtual(zf, sc) : a.empty_value;
          else if (RESID) { z[j] = drawn ? shade_virtual(zf, sc) : rs_vbg; thr[j] = drawn && THRESH ? cov_thr : a.max_diff; }
          else if (drawn && !TWO_KERNEL) thr[j] = THRESH ? shade_threshold(zf, sc, cov_thr) : shade_threshold(zf, sc);
#ifdef RTUF_COUNT
          if (drawn && r_px + j < a.width) atomicAdd(&count_words()[1], 1u);
#endif
        }
        flags4 = finish(ps, z, thr, frag, lab);
      } else {
        float z[4], thr[4];
        bool frag[4];
        uint32_t lab[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const unsigned long long k = keys[r_ly * kKeyStride + r_lx + j];
          frag[j] = true;
          thr[j] = thr_bg;
          lab[j] = 0u;
          if (RENDER && k == bgkey) z[j] = a.empty_value;
          else if (RESID && k == bgkey) { z[j] = rs_vbg; thr[j] = a.max_diff; frag[j] = analytic_bg; }
          else if (k == bgkey) { z[j] = bgz; frag[j] = analytic_bg; }
          else {                                        // the per-pixel division only runs where something was drawn
#ifdef RTUF_COUNT
            if (r_px + j < a.width) atomicAdd(&count_words()[1], 1u);
#endif
            // float z of the winner: written by the exact-z pass (rare), or (z24 + 1) * 2^-24 in the upper half of the depth
            // range, or -- only in tiles with near geometry (uniform test: the headline workload never gets there) -- from
            // z24 and the low bits of the float the key carries
            const uint32_t khi = (uint32_t)(k >> 32);
            if (!near_tile) {          // (uniform) no exact-z pass ran here, no depth below 0.51 exists
              z[j] = z_of_upper_half_z24(khi);
            } else if (k & kResolvedBit) {
              z[j] = __uint_as_float((uint32_t)k);
            } else {
              // (z24 + 1) * 2^-24 for z24 >= 2^23 - 1; smaller depths exist only in tiles with near geometry and take
              // near_z_from_key below.
              z[j] = z_of_upper_half_z24(khi);
              if (near_tile) {
                if (khi <= 8388608u) z[j] = near_z_from_key(khi, (uint32_t)k & kf.lowmask, kf.shift);
              }
            }
            if (!TWO_KERNEL && !THRESH && !RENDER && !RESID) thr[j] = shade_threshold(z[j], sc);
            // what the tables say of the winner's draw order (winner_order)
            if (LABELS && !THRESH) lab[j] = a.order_labels[winner_order(k, kf)];
            if (RESID) {                             // the winner's label, threshold and virtual depth
              const uint32_t ord = winner_order(k, kf);
              lab[j] = a.order_labels[ord];
              thr[j] = THRESH ? a.order_thr[ord] : a.max_diff;
              z[j] = shade_virtual(z[j], sc);
            } else if (THRESH) {
              const uint32_t ord = winner_order(k, kf);
              thr[j] = shade_threshold(z[j], sc, a.order_thr[ord]);
              if (LABELS) lab[j] = a.order_labels[ord];
            }
            if (RENDER) {                            // (draw order 0: the background quad drawn as geometry is background too)
              z[j] = winner_order(k, kf) ? shade_virtual(z[j], sc) : a.empty_value;
            }
          }
        }
        flags4 = finish(ps, z, thr, frag, lab);
      }
    }
    if (RESID) resid_reduce(rs_cls, rs_lab, rs_q, rs_rows, rs_tags, a.resid_table + (size_t)stream * (size_t)a.n_labels * 8u);
    if (BITS) {
      // 8 neighbouring lanes hold the 32 pixels of one output word (pixel x -> bit x % 32 of word x / 32 of its row):
      // OR their nibbles together (all lanes take part, invalid ones with 0) and let the group's first lane store
      uint32_t word = flags4 << (4 * (tid & 7));
      word |= (uint32_t)__shfl_xor((int)word, 1);
      word |= (uint32_t)__shfl_xor((int)word, 2);
      word |= (uint32_t)__shfl_xor((int)word, 4);
      if (valid && (tid & 7) == 0) {
        const int row_words = (a.width + 31) >> 5;
        const size_t wofs = ((size_t)stream * a.height + (size_t)(y_base + r_ly)) * (size_t)row_words + (size_t)(r_px >> 5);
        __builtin_nontemporal_store(word, a.bits + wofs);
      }
    }
  }
  if (BITS && __syncthreads_or(uncovered) && tid == 0) a.counters->shard[bin % kCounterShards].uncovered = 1u;
  if (RESID) {                               // the workgroup's rows go to the table: one 64-byte line per label it saw
    __syncthreads();
    if (tid < kResidSlots * 8) {
      const uint32_t tag = rs_tags[tid >> 3];
      const unsigned long long v = rs_rows[tid];
      if (tag != kResidFree && v != 0ull) atomicAdd(&a.resid_table[((size_t)stream * (size_t)a.n_labels + tag) * 8u + (uint32_t)(tid & 7)], v);
    }
  }
  RTUF_LANES_FLUSH(a.counters->shard[bin % kCounterShards]);
#ifdef RTUF_COUNT
  __syncthreads();
  if (!empty && tid == 0) {
    atomicAdd(&a.counters->shard[bin % kCounterShards].raster_atomics, (unsigned long long)count_words()[0]);
    atomicAdd(&a.counters->shard[bin % kCounterShards].drawn_pixels, (unsigned long long)count_words()[1]);
  }
#endif
}

// Registers: 7 waves/SIMD (72 VGPRs; seven workgroups' key tiles are 159.6 of the CU's 160 KB of LDS) for the variants
// without the cover pass -- the compiler spills two or three registers there and the kernel is still 5 % faster than at
// 6 waves/SIMD (80 VGPRs, where it needs 74: tile kernel 275 -> 261 us on the 256-stream VGA workload), the seventh
// workgroup per CU hides what the lanes wait for; the cover variants (walls: C4) were left at 6 up to round 5, where they
// measured the same alone and 2 % better beside the other lane's set-up kernel -- with the cover-only tiles resolved from
// registers (round 6) 7 is ahead there as well.  Left alone the compiler takes 84 registers = 5 waves/SIMD.
#ifndef RTUF_TILE_WAVES
#define RTUF_TILE_WAVES 7
#endif
#ifndef RTUF_TILE_WAVES_COVER
#define RTUF_TILE_WAVES_COVER 7      // (round 6, with the cover-only tiles off the key tile: 7 is 2.7 % ahead of 6 on C4's tile kernel, +0.7 % frames/s; up to round 5: 6)
#endif
// NT = threads of the workgroup: 256 (four waves per tile) for launches that fill the GPU; 1,024 (sixteen) for the small launches of
// one or a few camera streams, where the kernel's time is the serial window loop of its fullest tiles -- 150 workgroups for one
// VGA stream, each walking its bin 256 records at a time -- and more waves per tile shorten exactly that (one stream: raster
// stage 42 -> 23 us, 14.2 k -> 17.6 k frames/s; eight streams 98 k -> 109 k; profiles/r05_experiment_tile_threads.txt).
constexpr int kTileThreadsSmall = 1024;
template <bool TWO_KERNEL, bool U16, bool COVER, int NT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(COVER ? RTUF_TILE_WAVES_COVER : RTUF_TILE_WAVES))) void tile_kernel(TileArgs a) { tile_body<TWO_KERNEL ? TileOut::ZSurface : TileOut::Planes, U16, COVER, NT>(a); }
// mask-only output, one bit per pixel (rtuf_filter_batch_bits*): 4 (2) B/pixel in, 1/8 B/pixel out
template <bool U16, bool COVER, int NT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(COVER ? RTUF_TILE_WAVES_COVER : RTUF_TILE_WAVES))) void tile_bits_kernel(TileArgs a) { tile_body<TileOut::Bits, U16, COVER, NT>(a); }
// link labels beside the planes (rtuf_filter_batch*_labels): the variants of tile_kernel, plus 2 B/pixel out
#ifndef RTUF_TILE_WAVES_LABELS
#define RTUF_TILE_WAVES_LABELS 7
#endif
template <bool TWO_KERNEL, bool U16, bool COVER, int NT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(RTUF_TILE_WAVES_LABELS))) void tile_labels_kernel(TileArgs a) { tile_body<TWO_KERNEL ? TileOut::ZSurface : TileOut::Planes, U16, COVER, NT, true>(a); }
// per-link depth thresholds (rtuf_set_link_thresholds): the fused tile_kernel, tile_bits_kernel and tile_labels_kernel with
// one more gather (4 B, from the draw order -> threshold table) per drawn pixel
#ifndef RTUF_TILE_WAVES_THRESH
#define RTUF_TILE_WAVES_THRESH 7
#endif
template <bool U16, bool BITS, bool LABELS, bool COVER, int NT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(RTUF_TILE_WAVES_THRESH))) void tile_thresh_kernel(TileArgs a) { tile_body<BITS ? TileOut::Bits : TileOut::Planes, U16, COVER, NT, LABELS, true>(a); }
// virtual depth planes (rtuf_render_batch*): no sensor plane in, 4 (2) B/pixel out, plus 2 B/pixel with labels.
// Without the sensor registers the variants take 71 or 72 VGPRs and spill none at 7 waves/SIMD (the label variants' setting).
// More cannot help the 256-thread kernels: seven key tiles fill the CU's LDS, and seven workgroups of four waves are 7 per SIMD.
#ifndef RTUF_TILE_WAVES_RENDER
#define RTUF_TILE_WAVES_RENDER 7
#endif
template <bool U16, bool LABELS, bool COVER, int NT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(RTUF_TILE_WAVES_RENDER))) void tile_render_kernel(TileArgs a) { tile_body<TileOut::Render, U16, COVER, NT, LABELS>(a); }
// link residual tables (rtuf_link_residuals_batch*): 4 (2) B/pixel in, no plane out; 64 bytes per (stream, label) by atomics.
// 72 VGPRs without spills at 7 waves/SIMD for the 256-thread variants.  A 1,024-thread workgroup is four waves per SIMD and a
// second one would need eight, which 72 registers do not allow: those variants ask for 5 (up to 96 VGPRs) and lose nothing,
// where at 7 the cover variants among them spilled two registers.
#ifndef RTUF_TILE_WAVES_RESID
#define RTUF_TILE_WAVES_RESID 7
#endif
template <bool U16, bool THRESH, bool COVER, int NT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(NT > 256 ? 5 : RTUF_TILE_WAVES_RESID))) void tile_resid_kernel(TileArgs a) { tile_body<TileOut::Residual, U16, COVER, NT, false, THRESH>(a); }

// ---------------------------------------------------------------------------------------
// compare_kernel (two-kernel mode): streaming, 13 B/pixel (4 sensor + 4 z + 4 masked + 1 mask)
// ---------------------------------------------------------------------------------------

#ifndef RTUF_CMP_UNROLL
#define RTUF_CMP_UNROLL 1
#endif
constexpr int kCmpUnroll = RTUF_CMP_UNROLL;
template <bool U16>
__global__ __launch_bounds__(kBlock) void compare_kernel(CompareArgs a)
{
  ShadeConsts sc;
  sc.num = a.sc_num; sc.off = a.sc_off; sc.max_diff = a.max_diff; sc.replace_value = a.replace_value; sc.core = a.fast_div != 0;
  const size_t n4 = a.n_pixels >> 2;
  const uint16_t* in16 = reinterpret_cast<const uint16_t*>(a.depth);
  uint16_t* out16 = reinterpret_cast<uint16_t*>(a.masked);
  // No grid-stride loop: every workgroup takes kCmpUnroll * kBlock consecutive quads of pixels, so the workgroups in
  // flight form ONE compact front through the four arrays (a strided loop over 32 k workgroups had every lane jump
  // 134 MB per trip at 1,024 streams: 829 us instead of 640 for the same 4.09 GB).  All loads of a lane are issued
  // before the first is used.
  {
    const size_t i0 = (size_t)blockIdx.x * blockDim.x * kCmpUnroll + threadIdx.x;
    const size_t stride = blockDim.x;
    float sv[kCmpUnroll][4], zv[kCmpUnroll][4];
#pragma unroll
    for (int u = 0; u < kCmpUnroll; u++) {
      const size_t i = i0 + (size_t)u * stride;
      if (i >= n4) break;
      if (U16) {
        const ushort4 q = reinterpret_cast<const ushort4*>(in16)[i];
        sv[u][0] = u16_to_metres(q.x); sv[u][1] = u16_to_metres(q.y); sv[u][2] = u16_to_metres(q.z); sv[u][3] = u16_to_metres(q.w);
      } else {
        const float4 s = load_stream4(a.depth + 4 * i);
        sv[u][0] = s.x; sv[u][1] = s.y; sv[u][2] = s.z; sv[u][3] = s.w;
      }
      const float4 z = load_stream4(a.zsurface + 4 * i);      // (the tile kernel's z stores stay temporal: this read may still find them in MALL)
      zv[u][0] = z.x; zv[u][1] = z.y; zv[u][2] = z.z; zv[u][3] = z.w;
    }
#pragma unroll
    for (int u = 0; u < kCmpUnroll; u++) {
      const size_t i = i0 + (size_t)u * stride;
      if (i >= n4) break;
      float o[4];
      uint32_t mbits = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        bool f;
        o[j] = shade(sv[u][j], zv[u][j], sc, f);
        if (zv[u][j] != zv[u][j]) { o[j] = 0.0f; f = false; }
        if (f) mbits |= 0xffu << (8 * j);
      }
      if (U16) {
        store_stream4(out16 + 4 * i, metres_to_u16(o[0]), metres_to_u16(o[1]), metres_to_u16(o[2]), metres_to_u16(o[3]));
      } else {
        store_stream4(a.masked + 4 * i, o[0], o[1], o[2], o[3]);
      }
      if (a.mask) __builtin_nontemporal_store(mbits, reinterpret_cast<uint32_t*>(a.mask) + i);
    }
  }
  // tail
  if (blockIdx.x == 0 && threadIdx.x < (a.n_pixels & 3)) {
    const size_t i = (n4 << 2) + threadIdx.x;
    bool f;
    const float sen = U16 ? u16_to_metres(in16[i]) : a.depth[i];
    float o = shade(sen, a.zsurface[i], sc, f);
    if (a.zsurface[i] != a.zsurface[i]) { o = 0.0f; f = false; }
    if (U16) out16[i] = (uint16_t)metres_to_u16(o);
    else a.masked[i] = o;
    if (a.mask) a.mask[i] = f ? 255 : 0;
  }
}

// ---------------------------------------------------------------------------------------
// dilate_compare_kernel (silhouette dilation, rtuf_params.silhouette_dilation_px = r > 0): z-surface -> minimum over the
// (2r+1)^2 window of every pixel -> the compare kernel's outputs, or the bit-packed mask
// ---------------------------------------------------------------------------------------
// One workgroup per (64x32 output tile, stream of the launch group).  LDS holds the tile's z-surface with an r-pixel halo --
// columns from x0 - R4 (R4 = r rounded up to a multiple of 4, so every float4 of it is aligned), NaN outside the stream's
// image -- and then the row minima of the halo rows.  Both passes give a lane four outputs: the 2r - 2 inputs all four windows
// share are folded once, then the three each has of its own: (2r + 10) / 4 minimum instructions per output and pass instead of
// 2r + 1.  fminf returns the other operand when one is NaN, so NaN (nothing drawn, outside the image) is the identity and an
// all-NaN window gives NaN; the result is always one of the window's own values.  (r >= 1: at r = 0 the shared edges overlap.)
constexpr int kDilW = 64, kDilH = 32, kDilThreads = 256;
static_assert(kDilThreads == (kDilW / 4) * (kDilH / 2), "column pass and output: one lane per 4 x 2 pixels of the tile");
static_assert(kDilW % 32 == 0, "a tile row is whole mask-bit words");
__host__ __device__ constexpr int dilate_r4(int r) { return (r + 3) & ~3; }
static size_t dilate_lds_bytes(int r) { return (size_t)(kDilH + 2 * r) * (size_t)(kDilW + 2 * dilate_r4(r) + kDilW) * sizeof(float); }
static_assert((kDilH + 2 * kMaxDilation) * (kDilW + 2 * dilate_r4(kMaxDilation) + kDilW) * 4 <= 65536, "LDS of the largest radius");

__device__ __forceinline__ float4 fmin4(float4 a, float4 b) { return make_float4(fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z), fminf(a.w, b.w)); }

// The last step of dilate_compare_kernel and pad_compare_kernel (Args: DilateArgs or PadArgs): lane tid holds the window's z
// of tile rows ly and ly + 1, columns lx .. lx + 3, and shades exactly as compare_kernel does, with that z in place of the
// pixel's own.
template <bool U16, bool BITS, class Args>
__device__ __forceinline__ void shade_window_tile(const Args& a, const float4 (&zd)[2], int stream, int x0, int y0)
{
  const int tid = threadIdx.x, W = a.width, H = a.height;
  const int lx = (tid & 15) * 4, ly = (tid >> 4) * 2;
  ShadeConsts sc;
  sc.num = a.sc_num; sc.off = a.sc_off; sc.max_diff = a.max_diff; sc.replace_value = a.replace_value; sc.core = a.fast_div != 0;
  const bool vec = (W & 3) == 0;
  bool uncovered = false;                    // BITS: a pixel whose window holds nothing drawn
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int py = y0 + ly + i, px = x0 + lx;
    const bool valid = py < H && px < W;
    const float zz[4] = {zd[i].x, zd[i].y, zd[i].z, zd[i].w};
    uint32_t flags4 = 0;
    if (valid) {
      const size_t gofs = (size_t)stream * ((size_t)H * W) + (size_t)py * W + px;
      const int nvalid = min(4, W - px);
      float s[4];
      if (vec) {
        if (U16) {
          const ushort4 q = *reinterpret_cast<const ushort4*>(reinterpret_cast<const uint16_t*>(a.depth) + gofs);
          s[0] = u16_to_metres(q.x); s[1] = u16_to_metres(q.y); s[2] = u16_to_metres(q.z); s[3] = u16_to_metres(q.w);
        } else {
          const float4 v = load_stream4(a.depth + gofs);
          s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w;
        }
      } else {
        for (int j = 0; j < 4; j++)
          s[j] = j < nvalid ? (U16 ? u16_to_metres(reinterpret_cast<const uint16_t*>(a.depth)[gofs + j]) : a.depth[gofs + j]) : 0.0f;
      }
      float o[4];
      uint32_t mbits = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        bool f;
        o[j] = shade(s[j], zz[j], sc, f);
        if (zz[j] != zz[j]) { o[j] = 0.0f; f = false; if (BITS && j < nvalid) uncovered = true; }     // GL clear colour
        if (f) mbits |= (BITS ? 1u : 0xffu) << ((BITS ? 1 : 8) * j);
      }
      flags4 = mbits;
      if (!BITS) {
        if (vec) {
          if (U16) store_stream4(reinterpret_cast<uint16_t*>(a.masked) + gofs, metres_to_u16(o[0]), metres_to_u16(o[1]), metres_to_u16(o[2]), metres_to_u16(o[3]));
          else store_stream4(a.masked + gofs, o[0], o[1], o[2], o[3]);
          if (a.mask) __builtin_nontemporal_store(mbits, reinterpret_cast<uint32_t*>(a.mask + gofs));
        } else {
          for (int j = 0; j < nvalid; j++) {
            if (U16) reinterpret_cast<uint16_t*>(a.masked)[gofs + j] = (uint16_t)metres_to_u16(o[j]);
            else a.masked[gofs + j] = o[j];
            if (a.mask) a.mask[gofs + j] = (uint8_t)(mbits >> (8 * j));
          }
        }
      }
    }
    if (BITS) {
      // as tile_body: 8 neighbouring lanes hold the 32 pixels of one output word; OR their nibbles, the group's first lane stores
      uint32_t word = flags4 << (4 * (tid & 7));
      word |= (uint32_t)__shfl_xor((int)word, 1);
      word |= (uint32_t)__shfl_xor((int)word, 2);
      word |= (uint32_t)__shfl_xor((int)word, 4);
      if (valid && (tid & 7) == 0) {
        const int row_words = (W + 31) >> 5;
        const size_t wofs = ((size_t)stream * H + (size_t)py) * (size_t)row_words + (size_t)(px >> 5);
        __builtin_nontemporal_store(word, a.bits + wofs);
      }
    }
  }
  if (BITS) {
    const int bin = ((int)blockIdx.z * (int)gridDim.y + (int)blockIdx.y) * (int)gridDim.x + (int)blockIdx.x;
    if (__syncthreads_or(uncovered) && tid == 0) a.counters->shard[bin % kCounterShards].uncovered = 1u;
  }
}

template <bool U16, bool BITS>
__global__ __launch_bounds__(kDilThreads) void dilate_compare_kernel(DilateArgs a)
{
  extern __shared__ float dil_lds[];
  const int r = a.radius, R4 = dilate_r4(r);
  const int in_w = kDilW + 2 * R4;            // halo tile columns: image x = x0 - R4 + column
  const int rows = kDilH + 2 * r;             // halo tile rows:    image y = y0 - r + row
  float* zin = dil_lds;                       // [rows][in_w]
  float* rmin = dil_lds + rows * in_w;        // [rows][kDilW]  minimum over the row window of every output column
  const int tid = threadIdx.x;
  const int slot = blockIdx.z, stream = a.group_base + slot;
  const int x0 = blockIdx.x * kDilW, y0 = blockIdx.y * kDilH;
  const int W = a.width, H = a.height;
  const float nan = __uint_as_float(0x7fc00000u);
  const float* zs = a.zsurface + (size_t)slot * ((size_t)H * W);

  // 1. the halo tile (the window is clipped to the image, never padded: NaN is what the minimum ignores)
  if ((W & 3) == 0) {
    const int in_w4 = in_w >> 2;
    for (int i = tid; i < rows * in_w4; i += kDilThreads) {
      const int row = i / in_w4, c4 = i - row * in_w4;
      const int y = y0 - r + row, x = x0 - R4 + 4 * c4;
      float4 v = make_float4(nan, nan, nan, nan);
      if (y >= 0 && y < H && x >= 0 && x < W) v = *reinterpret_cast<const float4*>(zs + (size_t)y * W + x);      // (x < W: x + 3 < W)
      *reinterpret_cast<float4*>(zin + row * in_w + 4 * c4) = v;
    }
  } else {
    for (int i = tid; i < rows * in_w; i += kDilThreads) {
      const int row = i / in_w, c = i - row * in_w;
      const int y = y0 - r + row, x = x0 - R4 + c;
      float v = nan;
      if (y >= 0 && y < H && x >= 0 && x < W) v = zs[(size_t)y * W + x];
      zin[i] = v;
    }
  }
  __syncthreads();

  // 2. rows: outputs c .. c + 3 of a halo row; output c + j's window is p[j .. j + 2r]
  for (int i = tid; i < rows * (kDilW / 4); i += kDilThreads) {
    const int row = i >> 4, c = (i & 15) * 4;
    const float* p = zin + row * in_w + c + R4 - r;
    float core = nan;
    for (int k = 3; k <= 2 * r; k++) core = fminf(core, p[k]);
    const float e0 = p[0], e1 = p[1], e2 = p[2], f0 = p[2 * r + 1], f1 = p[2 * r + 2], f2 = p[2 * r + 3];
    *reinterpret_cast<float4*>(rmin + row * kDilW + c) =
        make_float4(fminf(core, fminf(e0, fminf(e1, e2))), fminf(core, fminf(e1, fminf(e2, f0))),
                    fminf(core, fminf(e2, fminf(f0, f1))), fminf(core, fminf(f0, fminf(f1, f2))));
  }
  __syncthreads();

  // 3. columns: tile rows ly and ly + 1, columns lx .. lx + 3; tile row y's window is halo rows y .. y + 2r
  const int lx = (tid & 15) * 4, ly = (tid >> 4) * 2;
  float4 zd[2];
  {
    const float* q = rmin + ly * kDilW + lx;
    float4 core = make_float4(nan, nan, nan, nan);
    for (int k = 1; k <= 2 * r; k++) core = fmin4(core, *reinterpret_cast<const float4*>(q + k * kDilW));
    zd[0] = fmin4(core, *reinterpret_cast<const float4*>(q));
    zd[1] = fmin4(core, *reinterpret_cast<const float4*>(q + (2 * r + 1) * kDilW));
  }

  // 4. shade exactly as compare_kernel does, with the window's z in place of the pixel's own
  shade_window_tile<U16, BITS>(a, zd, stream, x0, y0);
}

// ---------------------------------------------------------------------------------------
// pad_compare_kernel (link padding, rtuf_set_link_padding): z-surface + link slots -> per pixel the smallest z whose source
// reaches it -> the compare kernel's outputs, or the bit-packed mask
// ---------------------------------------------------------------------------------------
// One workgroup per (64x32 output tile, stream of the launch group), like dilate_compare_kernel.  The radius belongs to the
// SOURCE pixel here (R2 = link_padding_reach2 of its z and its link's padding), so the window is not separable into rows and
// columns; the kernel gathers, and keeps the cost proportional to what actually spreads:
//   1. the tile with a halo of kMaxLinkPaddingPx pixels goes to LDS as {z, R2} pairs, R2 computed once per halo pixel ({NaN, 0}
//      outside the image); a wave takes whole halo rows, so one ballot per row segment says whether the row holds a source
//      that spreads at all, and the waves reduce the halo's largest R2;
//   2. lane c of wave w owns column c of tile rows 8 w .. 8 w + 7, which start as their own z.  The wave walks the halo rows
//      within m = floor(sqrt(largest R2)) of its rows -- not 16 -- and skips those the ballots found empty; in a row its lanes
//      read neighbouring 8-byte pairs (one ds_read_b64 each, no two lanes of a half-wave on one bank) at the 2 m + 1 column
//      offsets, and a pair with R2 = 0 is tested against nothing (a wave whose 64 pairs are all 0 branches over the tests).
//      dx^2 + dy^2 <= R2 in integers; fminf keeps the other operand of a NaN.  A tile whose halo holds no R2 > 0 -- most of the
//      image -- has m = 0 and writes its own z straight through;
//   3. the minima go back to LDS (over the halo, which is dead by then) so that step 4 finds them in the layout it stores from;
//   4. shade_window_tile, as in dilate_compare_kernel.
constexpr int kPadR = kMaxLinkPaddingPx;
constexpr int kPadW = kDilW + 2 * kPadR, kPadH = kDilH + 2 * kPadR;      // the halo tile: image (x0 - kPadR + column, y0 - kPadR + row)
constexpr int kPadWaves = kDilThreads / 64, kPadRowsPerWave = kDilH / kPadWaves;
static_assert(kDilW == 64 && kDilH % kPadWaves == 0, "gather: a lane per tile column, a wave per strip of rows");
static_assert(kPadW * kPadH * 8 <= 49152 && kPadW * kPadH * 8 >= kDilW * kDilH * 4, "three workgroups per CU; the minima fit over the halo");

template <bool U16, bool BITS>
__global__ __launch_bounds__(kDilThreads) void pad_compare_kernel(PadArgs a)
{
  __shared__ uint2 halo[kPadH * kPadW];          // {bits of z, R2}
  __shared__ uint32_t row_spreads[kPadH];        // the halo row holds a pair with R2 > 0
  __shared__ uint32_t wave_max[kPadWaves];       // largest R2 of the rows a wave loaded
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slot = blockIdx.z, stream = a.group_base + slot;
  const int x0 = blockIdx.x * kDilW, y0 = blockIdx.y * kDilH;
  const int W = a.width, H = a.height;
  const float* zs = a.zsurface + (size_t)slot * ((size_t)H * W);
  const uint16_t* ss = a.slots + (size_t)slot * ((size_t)H * W);
  const float focal = a.focal[stream];

  // 1. the halo tile
  uint32_t mine = 0;
  for (int row = wave; row < kPadH; row += kPadWaves) {
    const int y = y0 - kPadR + row;
    bool spreads = false;
    for (int c0 = 0; c0 < kPadW; c0 += 64) {
      const int c = c0 + lane, x = x0 - kPadR + c;
      float z = __uint_as_float(0x7fc00000u);
      uint32_t r2 = 0;
      if (c < kPadW && y >= 0 && y < H && x >= 0 && x < W) {
        const size_t o = (size_t)y * W + x;
        z = zs[o];
        const uint32_t s = ss[o];
        if (s) r2 = link_padding_reach2(z, a.slot_pad[s], focal, a.sc_num, a.sc_off);
      }
      if (c < kPadW) halo[row * kPadW + c] = make_uint2(__float_as_uint(z), r2);
      spreads = spreads || __ballot(r2 != 0) != 0;
      mine = max(mine, r2);
    }
    if (lane == 0) row_spreads[row] = spreads ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine = max(mine, (uint32_t)__shfl_xor((int)mine, o));
  if (lane == 0) wave_max[wave] = mine;
  __syncthreads();
  uint32_t max_r2 = 0;
#pragma unroll
  for (int w = 0; w < kPadWaves; w++) max_r2 = max(max_r2, wave_max[w]);
  int m = 0;
  while ((uint32_t)((m + 1) * (m + 1)) <= max_r2) m++;      // (at most kPadR trips: R2 <= kPadR^2)

  // 2. gather: tile pixel (lane, ry0 + i) is halo pair (lane + kPadR, ry0 + i + kPadR)
  const int ry0 = wave * kPadRowsPerWave;
  float zmin[kPadRowsPerWave];
#pragma unroll
  for (int i = 0; i < kPadRowsPerWave; i++) zmin[i] = __uint_as_float(halo[(ry0 + i + kPadR) * kPadW + lane + kPadR].x);
  if (m > 0) {
    for (int sy = ry0 + kPadR - m; sy <= ry0 + kPadRowsPerWave - 1 + kPadR + m; sy++) {
      if (!row_spreads[sy]) continue;
      const uint2* src = halo + sy * kPadW + lane + kPadR;
      const int dy0 = sy - (ry0 + kPadR);          // to the strip's first row; row i: dy0 - i
      for (int dx = -m; dx <= m; dx++) {
        const uint2 v = src[dx];
        if (v.y) {
          const float z = __uint_as_float(v.x);
          const int dx2 = dx * dx;
#pragma unroll
          for (int i = 0; i < kPadRowsPerWave; i++)
            if ((uint32_t)(dx2 + (dy0 - i) * (dy0 - i)) <= v.y) zmin[i] = fminf(zmin[i], z);
        }
      }
    }
  }

  // 3. the minima, as a [kDilH][kDilW] tile
  __syncthreads();                                 // (every wave is done with the halo)
  float* zout = reinterpret_cast<float*>(halo);
#pragma unroll
  for (int i = 0; i < kPadRowsPerWave; i++) zout[(ry0 + i) * kDilW + lane] = zmin[i];
  __syncthreads();
  const int lx = (tid & 15) * 4, ly = (tid >> 4) * 2;
  float4 zd[2];
  zd[0] = *reinterpret_cast<const float4*>(zout + ly * kDilW + lx);
  zd[1] = *reinterpret_cast<const float4*>(zout + (ly + 1) * kDilW + lx);

  // 4. shade exactly as compare_kernel does, with the reaching z in place of the pixel's own
  shade_window_tile<U16, BITS>(a, zd, stream, x0, y0);
}

// A batch's counters (one block per launch group) go to pinned host memory with plain stores from a tiny kernel, one
// workgroup per block: a hipMemcpyAsync of 8 KB costs a blit launch plus ~10 us of copy-engine set-up on the stream.
// Every raster lane publishes the blocks of its own groups (first, first + stride, ...) at the end of its part of the batch.
// It is the last kernel a lane runs for a launch group, and it sees every counter the host will judge the batch by when it
// retires it: it makes the same judgement on the device and leaves it in the batch slot's status word, for consumers that read
// the output planes on a stream of their own (rtuf_order_stream_after_batches) before the host has retired the batch.
__global__ void publish_counters_kernel(const Counters* __restrict__ src, Counters* __restrict__ host_dst, int first, int stride,
                                        uint32_t* status, PublishLimits lim)
{
  const int b = first + (int)blockIdx.x * stride;
  const uint4* s = reinterpret_cast<const uint4*>(src + b);
  uint4* d = reinterpret_cast<uint4*>(host_dst + b);
  for (int i = threadIdx.x; i < (int)(sizeof(Counters) / 16); i += blockDim.x) d[i] = s[i];
  if (threadIdx.x < 64) {            // the first wave: a shard per lane (kCounterShards <= 64)
    uint32_t f = 0;
    for (int i = threadIdx.x; i < kCounterShards; i += 64) {
      const CounterShard& sh = src[b].shard[i];
      if (sh.max_bin_fill > lim.capacity || sh.max_fbin_fill > lim.fcapacity) f |= kStatusBinOverflow;
      if (sh.clip_overflow) f |= kStatusClipOverflow;
      if (sh.max_big_fill > lim.big_capacity) f |= kStatusBigOverflow;
      if (sh.uncovered) f |= kStatusUncovered;
    }
    if (threadIdx.x == 0 && src[b].work.n_items > src[b].work.grid) f |= kStatusGridShort;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) f |= (uint32_t)__shfl_xor((int)f, o);
    if (threadIdx.x == 0) {
      if (f) atomicOr(status, f);
      __threadfence();               // the flags are visible before this group counts as finished
      atomicSub(status, 1u);
    }
  }
}

// bin headers of a fresh (or regrown) working set: nothing binned, no cover
__global__ void init_headers_kernel(BinHeader* hdr, size_t n_bins)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_bins) *reinterpret_cast<uint4*>(hdr + i) = make_uint4(0u, 0u, 0xffffffffu, 0xffffffffu);
}

// One wave that does nothing for `ticks` of the constant-rate clock: rtuf_create uses two of them to find out whether two HIP
// streams can run side by side (the runtime multiplexes streams onto a few hardware queues, and two streams that share a
// queue run their kernels one after the other).
__global__ void spin_kernel(unsigned long long ticks)
{
  const unsigned long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}
void launch_spin(unsigned long long ticks, hipStream_t st) { hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, st, ticks); }

// host-callable launchers ---------------------------------------------------------------
void launch_publish_counters(const Counters* src, Counters* host_dst, int first, int stride, int count, uint32_t* status, PublishLimits lim, hipStream_t st)
{
  if (count > 0) hipLaunchKernelGGL(publish_counters_kernel, dim3((unsigned)count), dim3(256), 0, st, src, host_dst, first, stride, status, lim);
}
void launch_init_headers(BinHeader* hdr, size_t n_bins, hipStream_t st)
{
  hipLaunchKernelGGL(init_headers_kernel, dim3((unsigned)((n_bins + 255) / 256)), dim3(256), 0, st, hdr, n_bins);
}
void launch_fk(const FkArgs& a, hipStream_t st)
{
  if (a.n_frames <= kFkMaxFrames) {
    const int threads = a.n_frames <= 64 ? 64 : (a.n_frames <= 128 ? 128 : kFkMaxFrames);
    hipLaunchKernelGGL(fk_tree_kernel, dim3(a.n_streams), dim3(threads), 0, st, a);
    return;
  }
  const int total = a.n_streams * (a.n_links_model + 1);
  hipLaunchKernelGGL(fk_kernel, dim3((total + 63) / 64), dim3(64), 0, st, a);
}
void launch_pose(const PoseArgs& a, hipStream_t st)
{
  const int total = a.n_streams * (a.n_draws + 1);
  hipLaunchKernelGGL(pose_kernel, dim3((total + 127) / 128), dim3(128), 0, st, a);
}
void launch_cull(const SetupArgs& a, hipStream_t st)
{
  hipLaunchKernelGGL(cull_kernel, dim3(a.n_chunks), dim3(kBlock), 0, st, a);
}
uint32_t launch_setup(const SetupArgs& a, uint32_t items_hint, bool sweep, hipStream_t st)
{
  // The work-list length is only known on the device.  The grid is sized from the previous batch's
  // length (+25 %; robot and camera move little between frames).  Without a hint: the worst case (every
  // chunk visible in every stream).  Neighbouring workgroups take neighbouring items, which share a
  // chunk's geometry in L2.  If the list may be longer than the grid, either a small strided launch of
  // the same code sweeps the remainder (sweep = true), or the caller compares the returned grid size
  // with the list length it reads back and runs the batch again (a wrong guess costs time, never pixels).
  const long long worst = (long long)a.n_chunks * max_items_per_chunk(a.group_size);
  long long grid = worst;
  if (items_hint) grid = std::min<long long>(worst, (long long)items_hint + items_hint / 4 + 64);
  hipLaunchKernelGGL(setup_kernel<false>, dim3((unsigned)grid), dim3(kBlock), 0, st, a, 0u);
  if (grid < worst && sweep) hipLaunchKernelGGL(setup_kernel<true>, dim3(256), dim3(kBlock), 0, st, a, (uint32_t)grid);
  return (uint32_t)grid;
}
// workgroups per counter shard: enough to take the shard's whole list in one pass, at most kClipGridWgs (a context of one
// camera stream launches 8 per shard and holds an 8-MiB spill area instead of 64 MiB)
static int clip_wgs_per_shard(uint32_t clip_capacity) { return (int)std::min<uint32_t>((clip_capacity + kClipBlock - 1) / kClipBlock, (uint32_t)kClipGridWgs); }
void launch_clip(const SetupArgs& a, hipStream_t st)
{
  // the item count lives on the device: fixed grid, grid-stride loop
  hipLaunchKernelGGL(clip_kernel, dim3(kCounterShards * clip_wgs_per_shard(a.clip_capacity)), dim3(kClipBlock), 0, st, a);
}
size_t clip_spill_bytes(uint32_t clip_capacity) { return (size_t)(kClipMaxV - kClipLdsV) * kCounterShards * clip_wgs_per_shard(clip_capacity) * kClipBlock * sizeof(float4); }
void launch_bigrec(const SetupArgs& a, bool cover_pass, hipStream_t st)
{
  // the list lengths live on the device: fixed grid, kBigWavesPerShard waves per shard, each strides over its shard's list
  if (cover_pass) hipLaunchKernelGGL(bigrec_kernel<0>, dim3(kCounterShards * kBigWavesPerShard / 4), dim3(256), 0, st, a);
  hipLaunchKernelGGL(bigrec_kernel<1>, dim3(kCounterShards * kBigWavesPerShard / 4), dim3(256), 0, st, a);
}
#ifndef RTUF_SMALL_LAUNCH
#define RTUF_SMALL_LAUNCH 2048     // launches of fewer tile workgroups than this take the 1,024-thread kernels (0: never)
#endif
// (RTUF_SMALL_LAUNCH in the environment overrides the built-in threshold: the tests run their small scenes through both kernels)
static long long small_launch_threshold()
{
  static const long long t = [] { const char* e = getenv("RTUF_SMALL_LAUNCH"); return e && *e ? atoll(e) : (long long)RTUF_SMALL_LAUNCH; }();
  return t;
}
// A variant's instantiation, for one workgroup size and with or without the cover code: every legal variant (rtuf_routes.h) is
// one case below, once -- the compiler refuses a second -- and anything else is no kernel.  V's arguments read as TileVariant's
// fields: output, labels, thresh, u16.
using TileKernel = void (*)(TileArgs);
template <bool COVER, int NT>
static TileKernel tile_kernel_for(TileVariant v)
{
  using O = TileOut;
  constexpr auto V = [](TileOut out, bool labels, bool thresh, bool u16) { return tile_variant_index(TileVariant{out, labels, thresh, u16, COVER}); };
  switch (tile_variant_index(TileVariant{v.out, v.labels, v.thresh, v.u16, COVER})) {
    case V(O::Residual, false, true, true): return tile_resid_kernel<true, true, COVER, NT>;
    case V(O::Residual, false, true, false): return tile_resid_kernel<false, true, COVER, NT>;
    case V(O::Residual, false, false, true): return tile_resid_kernel<true, false, COVER, NT>;
    case V(O::Residual, false, false, false): return tile_resid_kernel<false, false, COVER, NT>;
    case V(O::Render, true, false, true): return tile_render_kernel<true, true, COVER, NT>;
    case V(O::Render, true, false, false): return tile_render_kernel<false, true, COVER, NT>;
    case V(O::Render, false, false, true): return tile_render_kernel<true, false, COVER, NT>;
    case V(O::Render, false, false, false): return tile_render_kernel<false, false, COVER, NT>;
    case V(O::Planes, true, true, true): return tile_thresh_kernel<true, false, true, COVER, NT>;
    case V(O::Planes, true, true, false): return tile_thresh_kernel<false, false, true, COVER, NT>;
    case V(O::Bits, false, true, true): return tile_thresh_kernel<true, true, false, COVER, NT>;
    case V(O::Bits, false, true, false): return tile_thresh_kernel<false, true, false, COVER, NT>;
    case V(O::Planes, false, true, true): return tile_thresh_kernel<true, false, false, COVER, NT>;
    case V(O::Planes, false, true, false): return tile_thresh_kernel<false, false, false, COVER, NT>;
    case V(O::ZSurface, true, false, false): return tile_labels_kernel<true, false, COVER, NT>;
    case V(O::Planes, true, false, true): return tile_labels_kernel<false, true, COVER, NT>;
    case V(O::Planes, true, false, false): return tile_labels_kernel<false, false, COVER, NT>;
    case V(O::Bits, false, false, true): return tile_bits_kernel<true, COVER, NT>;
    case V(O::Bits, false, false, false): return tile_bits_kernel<false, COVER, NT>;
    case V(O::ZSurface, false, false, false): return tile_kernel<true, false, COVER, NT>;
    case V(O::Planes, false, false, true): return tile_kernel<false, true, COVER, NT>;
    case V(O::Planes, false, false, false): return tile_kernel<false, false, COVER, NT>;
    default: return nullptr;
  }
}
bool launch_tile(const TileArgs& a, TileVariant v, hipStream_t st)
{
  const bool small = (long long)a.tiles_x * a.tiles_y * a.group_size < small_launch_threshold();
  const TileKernel kernel = small ? (v.cover ? tile_kernel_for<true, kTileThreadsSmall>(v) : tile_kernel_for<false, kTileThreadsSmall>(v))
                                  : (v.cover ? tile_kernel_for<true, kTileThreads>(v) : tile_kernel_for<false, kTileThreads>(v));
  if (!kernel) return false;
  hipLaunchKernelGGL(kernel, dim3(a.tiles_x, a.tiles_y, a.group_size), dim3(small ? kTileThreadsSmall : kTileThreads), 0, st, a);
  return true;
}
// A launch group's rows of a residual table start from zero on every run.  (A kernel, not hipMemsetAsync: the memset node a
// stream capture makes of it filled the rows with other values when the graph was replayed.)
__global__ __launch_bounds__(kBlock) void zero_words_kernel(unsigned long long* p, size_t n)
{
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) p[i] = 0ull;
}
void launch_zero_residual_rows(unsigned long long* rows, size_t n_words, hipStream_t st)
{
  const size_t blocks = (n_words + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks))), dim3(kBlock), 0, st, rows, n_words);
}
void launch_compare(const CompareArgs& a, hipStream_t st)
{
  size_t n4 = a.n_pixels >> 2;
  size_t blocks = (n4 + (size_t)kBlock * kCmpUnroll - 1) / ((size_t)kBlock * kCmpUnroll);
  if (blocks == 0) blocks = 1;
  if (a.io_u16) hipLaunchKernelGGL(compare_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
  else hipLaunchKernelGGL(compare_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
}
void launch_dilate_compare(const DilateArgs& a, hipStream_t st)
{
  const dim3 grid((unsigned)((a.width + kDilW - 1) / kDilW), (unsigned)((a.height + kDilH - 1) / kDilH), (unsigned)a.group_size);
  const size_t lds = dilate_lds_bytes(a.radius);
  if (a.bits) {
    if (a.io_u16) hipLaunchKernelGGL((dilate_compare_kernel<true, true>), grid, dim3(kDilThreads), lds, st, a);
    else hipLaunchKernelGGL((dilate_compare_kernel<false, true>), grid, dim3(kDilThreads), lds, st, a);
  } else if (a.io_u16) hipLaunchKernelGGL((dilate_compare_kernel<true, false>), grid, dim3(kDilThreads), lds, st, a);
  else hipLaunchKernelGGL((dilate_compare_kernel<false, false>), grid, dim3(kDilThreads), lds, st, a);
}
void launch_pad_compare(const PadArgs& a, hipStream_t st)
{
  const dim3 grid((unsigned)((a.width + kDilW - 1) / kDilW), (unsigned)((a.height + kDilH - 1) / kDilH), (unsigned)a.group_size);
  if (a.bits) {
    if (a.io_u16) hipLaunchKernelGGL((pad_compare_kernel<true, true>), grid, dim3(kDilThreads), 0, st, a);
    else hipLaunchKernelGGL((pad_compare_kernel<false, true>), grid, dim3(kDilThreads), 0, st, a);
  } else if (a.io_u16) hipLaunchKernelGGL((pad_compare_kernel<true, false>), grid, dim3(kDilThreads), 0, st, a);
  else hipLaunchKernelGGL((pad_compare_kernel<false, false>), grid, dim3(kDilThreads), 0, st, a);
}

// ---- filtered point clouds (include/rtuf.h, FILTERED POINT CLOUDS) ------------------------------------------------------
// A cloud batch is a mask-bits batch: the kernels below run behind the launch group's tile (or dilate) kernel on its lane,
// read the bits it wrote and the sensor planes once more, and write the points.  Nothing here is atomic and no result
// depends on the order of execution: the compacted form is counted, scanned and scattered in row-major order.

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kCloudNaN = 0x7fc00000u;      // what a pixel without a point holds in the organized form

// Organized form: one lane per four pixels of a row -- one 16-byte (f32) or 8-byte (16UC1) sensor load, the group's nibble of
// its bits word, three 16-byte non-temporal stores (48 contiguous bytes).  grid: (ceil(H * W/4 / kBlock), group_size).
template <bool U16>
__global__ __launch_bounds__(kBlock) void cloud_organized_kernel(CloudArgs a)
{
  const int w4 = a.width >> 2;
  const uint32_t t = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (t >= (uint32_t)w4 * (uint32_t)a.height) return;
  const int stream = a.group_base + (int)blockIdx.y;
  const int v = (int)(t / (uint32_t)w4), u = (int)(t - (uint32_t)v * (uint32_t)w4) * 4;
  const size_t pix = (size_t)stream * (size_t)a.width * (size_t)a.height + (size_t)t * 4u;      // (rows are contiguous: W = 4 * w4)
  float s[4];
  if (U16) {
    const uint2 q = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(a.depth) + pix);
    s[0] = u16_to_metres(q.x & 0xffffu); s[1] = u16_to_metres(q.x >> 16); s[2] = u16_to_metres(q.y & 0xffffu); s[3] = u16_to_metres(q.y >> 16);
  } else {
    const float4 q = *reinterpret_cast<const float4*>(a.depth + pix);
    s[0] = q.x; s[1] = q.y; s[2] = q.z; s[3] = q.w;
  }
  const int row_words = (a.width + 31) >> 5;
  const uint32_t nib = a.bits[((size_t)stream * a.height + (size_t)v) * (size_t)row_words + (size_t)(u >> 5)] >> (u & 31);
  const CloudIntrinsics k = a.intr[stream];
  float p[12];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    float x, y, z;
    cloud_point(u + j, v, s[j], k, x, y, z);
    const bool kept = !((nib >> j) & 1u) && cloud_sensor_valid(s[j]);
    p[3 * j] = kept ? x : __uint_as_float(kCloudNaN);
    p[3 * j + 1] = kept ? y : __uint_as_float(kCloudNaN);
    p[3 * j + 2] = kept ? z : __uint_as_float(kCloudNaN);
  }
  f32x4* dst = reinterpret_cast<f32x4*>(a.points + pix * 3u);
#pragma unroll
  for (int j = 0; j < 3; j++) {
    f32x4 o;
    o.x = p[4 * j]; o.y = p[4 * j + 1]; o.z = p[4 * j + 2]; o.w = p[4 * j + 3];
    __builtin_nontemporal_store(o, dst + j);
  }
}

// One 64-pixel chunk of a row, a pixel per lane (the last chunk of a row is partial when W % 64 != 0): the coalesced sensor
// load, the pixel's bit of the chunk's two bits words, and the wave's ballot of the kept pixels.
template <bool U16>
__device__ __forceinline__ unsigned long long cloud_chunk(const CloudArgs& a, size_t row_pix, const uint32_t* row_bits, int u, float& s)
{
  bool kept = false;
  s = 0.0f;
  if (u < a.width) {
    s = U16 ? u16_to_metres(reinterpret_cast<const uint16_t*>(a.depth)[row_pix + (size_t)u]) : a.depth[row_pix + (size_t)u];
    kept = !((row_bits[u >> 5] >> (u & 31)) & 1u) && cloud_sensor_valid(s);
  }
  return __ballot(kept);
}

// Compacted form, step 1: one wave per (stream, row) counts the row's kept pixels; lane 0 stores the count.
template <bool U16>
__global__ __launch_bounds__(kBlock) void cloud_row_count_kernel(CloudArgs a)
{
  const uint32_t wave = (blockIdx.x * (uint32_t)kBlock + threadIdx.x) >> 6;
  if (wave >= (uint32_t)a.group_size * (uint32_t)a.height) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int sl = (int)(wave / (uint32_t)a.height), v = (int)(wave - (uint32_t)sl * (uint32_t)a.height), stream = a.group_base + sl;
  const size_t row = (size_t)stream * a.height + (size_t)v;
  const uint32_t* row_bits = a.bits + row * (size_t)((a.width + 31) >> 5);
  uint32_t total = 0;
  for (int c0 = 0; c0 < a.width; c0 += 64) {
    float s;
    total += (uint32_t)__popcll(cloud_chunk<U16>(a, row * (size_t)a.width, row_bits, c0 + lane, s));
  }
  if (lane == 0) a.row_count[row] = total;
}

// Step 2: one workgroup per stream, the exclusive scan of its H row counts (any H: kBlock rows per trip and a carry) and the
// stream's total.
__global__ __launch_bounds__(kBlock) void cloud_scan_kernel(CloudArgs a)
{
  __shared__ uint32_t s_wave[kBlock / 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int stream = a.group_base + (int)blockIdx.x;
  const uint32_t* rc = a.row_count + (size_t)stream * a.height;
  uint32_t* rs = a.row_start + (size_t)stream * a.height;
  uint32_t carry = 0;
  for (int base = 0; base < a.height; base += kBlock) {
    const int i = base + tid;
    const uint32_t x = i < a.height ? rc[i] : 0u;
    uint32_t inc = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)inc, o);
      if (lane >= o) inc += y;
    }
    if (lane == 63) s_wave[wid] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; w++) { const uint32_t t = s_wave[w]; before += w < wid ? t : 0u; all += t; }
    if (i < a.height) rs[i] = carry + before + inc - x;
    carry += all;
    __syncthreads();
  }
  if (tid == 0) a.counts[stream] = carry;
}

// Step 3: the shape of the count kernel again.  Per chunk a kept pixel's place is the row's start + the kept pixels of the
// row's earlier chunks + those of the lanes below it; places at or beyond the capacity are not written.
template <bool U16>
__global__ __launch_bounds__(kBlock) void cloud_emit_kernel(CloudArgs a)
{
  const uint32_t wave = (blockIdx.x * (uint32_t)kBlock + threadIdx.x) >> 6;
  if (wave >= (uint32_t)a.group_size * (uint32_t)a.height) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int sl = (int)(wave / (uint32_t)a.height), v = (int)(wave - (uint32_t)sl * (uint32_t)a.height), stream = a.group_base + sl;
  const size_t row = (size_t)stream * a.height + (size_t)v;
  const uint32_t* row_bits = a.bits + row * (size_t)((a.width + 31) >> 5);
  const CloudIntrinsics k = a.intr[stream];
  const uint32_t capacity = (uint32_t)a.capacity;
  uint32_t running = a.row_start[row];
  for (int c0 = 0; c0 < a.width && running < capacity; c0 += 64) {
    float s;
    const int u = c0 + lane;
    const unsigned long long m = cloud_chunk<U16>(a, row * (size_t)a.width, row_bits, u, s);
    const uint32_t dst = running + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (((m >> lane) & 1ull) && dst < capacity) {
      float x, y, z;
      cloud_point(u, v, s, k, x, y, z);
      float* p = a.points + ((size_t)stream * capacity + dst) * 3u;
      p[0] = x; p[1] = y; p[2] = z;
      if (a.index) a.index[(size_t)stream * capacity + dst] = (uint32_t)(v * a.width + u);
    }
    running += (uint32_t)__popcll(m);
  }
}

void launch_cloud(const CloudArgs& a, hipStream_t st)
{
  if (a.capacity <= 0) {
    const dim3 grid((unsigned)(((size_t)(a.width >> 2) * a.height + kBlock - 1) / kBlock), (unsigned)a.group_size);
    if (a.io_u16) hipLaunchKernelGGL(cloud_organized_kernel<true>, grid, dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL(cloud_organized_kernel<false>, grid, dim3(kBlock), 0, st, a);
    return;
  }
  // a wave per (stream, row): batch = 1 still spreads its H rows over the GPU
  const unsigned row_blocks = (unsigned)(((size_t)a.group_size * a.height * 64u + kBlock - 1) / kBlock);
  if (a.io_u16) hipLaunchKernelGGL(cloud_row_count_kernel<true>, dim3(row_blocks), dim3(kBlock), 0, st, a);
  else hipLaunchKernelGGL(cloud_row_count_kernel<false>, dim3(row_blocks), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(cloud_scan_kernel, dim3((unsigned)a.group_size), dim3(kBlock), 0, st, a);
  if (a.io_u16) hipLaunchKernelGGL(cloud_emit_kernel<true>, dim3(row_blocks), dim3(kBlock), 0, st, a);
  else hipLaunchKernelGGL(cloud_emit_kernel<false>, dim3(row_blocks), dim3(kBlock), 0, st, a);
}


// ---- link clearance tables (include/rtuf.h, LINK CLEARANCE TABLES) -------------------------------------------------------
// A clearance batch is a mask-bits batch too: behind the launch group's tile (or dilate) kernel its lane poses the spheres of
// the group's streams, sets the group's rows to "nothing", takes per (stream, label) the minimum of {clearance, pixel} and the
// number of kept points within max_distance over all (kept point, sphere) pairs, and turns the rows into rtuf_link_clearance.
// Minima and integer counts only: no result depends on the order of execution, and the box culling below is conservative.

constexpr unsigned long long kClearanceNone = ~0ull;      // a row's key while no pair is within max_distance

// One lane per (stream, sphere): centre in the camera frame and radius; radius -1 where the stream does not render the model.
__global__ __launch_bounds__(kBlock) void clearance_spheres_kernel(ClearanceArgs a)
{
  const uint32_t t = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (t >= (uint32_t)a.n_spheres) return;
  const int stream = a.group_base + (int)blockIdx.y;
  const ClearanceSphere sp = a.spheres[t];
  float4 o = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
  if ((a.model_mask[stream] >> sp.model) & 1ull) {
    const float c[3] = {sp.x, sp.y, sp.z};
    float out[3];
    const Camera* cam = a.cams + stream;
    clearance_centre(a.link_tf + ((size_t)stream * (size_t)a.n_links + sp.link) * 16u, cam->cam_tf, cam->offset_inv, c, out);
    o = make_float4(out[0], out[1], out[2], sp.r);
  }
  a.posed[(size_t)stream * (size_t)a.n_spheres + t] = o;
}

// The group's rows start from {no key, count 0} on every run, re-run and replay.  (A kernel, not a captured memset: see
// zero_words_kernel.)
__global__ __launch_bounds__(kBlock) void clearance_zero_kernel(unsigned long long* rows, size_t n_rows)
{
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_rows; i += (size_t)gridDim.x * kBlock) {
    rows[2 * i] = kClearanceNone;
    rows[2 * i + 1] = 0ull;
  }
}

__device__ __forceinline__ float clr_wave_min(float v)
{
#pragma unroll
  for (int o = 32; o; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float clr_wave_max(float v)
{
#pragma unroll
  for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ unsigned long long clr_wave_min_u64(unsigned long long v)
{
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
    const unsigned long long w = ((unsigned long long)hi << 32) | lo;
    v = w < v ? w : v;
  }
  return v;
}
__device__ __forceinline__ float clr_uniform(float v) { return __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(v))); }

// One wave per 64-pixel chunk of a row (cloud_chunk's pixels), four chunks per workgroup, all of one stream.  The stream's posed
// spheres pass through LDS in trips of kClearanceTrip; every wave with a kept point walks them in label order, skips a sphere
// whose distance to the wave's box of points is beyond max_distance + r by more than the arithmetic could be wrong, and keeps
// per lane the smallest key {order bits of the clearance, pixel} of the label's pairs within max_distance.  Where the label
// changes the wave's minimum and its number of lanes with such a pair go to the workgroup's LDS rows; the rows the workgroup
// touched go to the table at the end: one 64-bit atomicMin and one atomicAdd each.  Row 0 takes every label's pairs.
template <bool U16>
__global__ __launch_bounds__(kBlock) void clearance_kernel(ClearanceArgs a)
{
  __shared__ float4 s_sph[kClearanceTrip];
  __shared__ uint32_t s_slot[kClearanceTrip];
  __shared__ unsigned long long s_key[kMaxClearanceLabels + 1];
  __shared__ uint32_t s_cnt[kMaxClearanceLabels + 1];
  const int tid = (int)threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int stream = a.group_base + (int)blockIdx.y;
  const int cpr = (a.width + 63) >> 6;                      // chunks per row
  const uint32_t w = blockIdx.x * (uint32_t)(kBlock / 64) + (uint32_t)wid;
  for (int i = tid; i <= a.n_slots; i += kBlock) { s_key[i] = kClearanceNone; s_cnt[i] = 0u; }
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  bool kept = false;
  uint32_t pixel = 0;
  if (w < (uint32_t)a.height * (uint32_t)cpr) {
    const int v = (int)(w / (uint32_t)cpr), u = (int)(w - (uint32_t)v * (uint32_t)cpr) * 64 + lane;
    if (u < a.width) {
      const size_t row = (size_t)stream * a.height + (size_t)v;
      const size_t pix = row * (size_t)a.width + (size_t)u;
      const float s = U16 ? u16_to_metres(reinterpret_cast<const uint16_t*>(a.depth)[pix]) : a.depth[pix];
      const uint32_t word = a.bits[row * (size_t)((a.width + 31) >> 5) + (size_t)(u >> 5)];
      kept = !((word >> (u & 31)) & 1u) && cloud_sensor_valid(s);
      cloud_point(u, v, s, a.intr[stream], px, py, pz);
      pixel = (uint32_t)(v * a.width + u);
    }
  }
  const bool any = __ballot(kept) != 0ull;                  // (wave-uniform)
  // a workgroup without a kept point stages no sphere and touches no row (the barrier also publishes the rows' initial values)
  if (!__syncthreads_or(any ? 1 : 0)) return;
  const float inf = __uint_as_float(0x7f800000u);
  const float lox = clr_wave_min(kept ? px : inf), loy = clr_wave_min(kept ? py : inf), loz = clr_wave_min(kept ? pz : inf);
  const float hix = clr_wave_max(kept ? px : -inf), hiy = clr_wave_max(kept ? py : -inf), hiz = clr_wave_max(kept ? pz : -inf);
  unsigned long long best = kClearanceNone, best0 = kClearanceNone;
  bool hit = false, hit0 = false;
  int cur_slot = -1;
  auto flush = [&](int row, unsigned long long& b, bool& h) {
    const unsigned long long m = __ballot(h);
    if (m) {
      const unsigned long long k = clr_wave_min_u64(b);
      if (lane == 0) { atomicMin(&s_key[row], k); atomicAdd(&s_cnt[row], (uint32_t)__popcll(m)); }
    }
    b = kClearanceNone; h = false;
  };
  for (int t0 = 0; t0 < a.n_spheres; t0 += kClearanceTrip) {
    const int nt = min(kClearanceTrip, a.n_spheres - t0);
    __syncthreads();                         // (the rows are initialised; every wave is done with the trip before)
    for (int i = tid; i < nt; i += kBlock) {
      s_sph[i] = a.posed[(size_t)stream * (size_t)a.n_spheres + (size_t)(t0 + i)];
      s_slot[i] = a.spheres[t0 + i].label_slot >> 16;
    }
    __syncthreads();
    if (!any) continue;
    for (int j = 0; j < nt; j++) {
      const float4 q = s_sph[j];
      const float cx = clr_uniform(q.x), cy = clr_uniform(q.y), cz = clr_uniform(q.z), r = clr_uniform(q.w);
      if (r < 0.0f) continue;                // the stream does not render this sphere's model
      const int slot = __builtin_amdgcn_readfirstlane((int)s_slot[j]);
      if (slot != cur_slot) {
        if (cur_slot >= 0) flush(cur_slot + 1, best, hit);
        cur_slot = slot;
      }
      // distance from the centre to the box of the wave's kept points: no point of the wave is nearer.  A computed clearance
      // is below max_distance only if the computed distance is below (max_distance + r)(1 + 2^-23); distance and bound carry
      // a few rounding errors of 2^-24 each: a margin of a thousandth is far beyond them (and +inf never rejects)
      const float ex = fmaxf(fmaxf(lox - cx, cx - hix), 0.0f), ey = fmaxf(fmaxf(loy - cy, cy - hiy), 0.0f), ez = fmaxf(fmaxf(loz - cz, cz - hiz), 0.0f);
      const float bound = sqrtf((ex * ex + ey * ey) + ez * ez);
      if (bound > (a.max_distance + r) * 1.001f + 1e-30f) continue;
      const float c = clearance_point_sphere(px, py, pz, cx, cy, cz, r);
      if (kept && c < a.max_distance) {
        const unsigned long long key = ((unsigned long long)clearance_order_bits(c) << 32) | pixel;
        best = key < best ? key : best; hit = true;
        best0 = key < best0 ? key : best0; hit0 = true;
      }
    }
  }
  if (any) {
    if (cur_slot >= 0) flush(cur_slot + 1, best, hit);
    flush(0, best0, hit0);
  }
  __syncthreads();
  for (int i = tid; i <= a.n_slots; i += kBlock) {
    const uint32_t cnt = s_cnt[i];
    if (!cnt) continue;
    const uint32_t label = i ? a.slot_label[i - 1] : 0u;
    unsigned long long* row = a.table + ((size_t)stream * (size_t)a.n_labels + label) * 2u;
    atomicMin(row, s_key[i]);
    atomicAdd(reinterpret_cast<uint32_t*>(row + 1), cnt);
  }
}

// One wave per (stream, label): the row's key becomes clearance and pixel, and the sphere is the smallest id among the row's
// spheres (row 0: all of them) that give exactly that clearance at that pixel.
template <bool U16>
__global__ __launch_bounds__(kBlock) void clearance_finish_kernel(ClearanceArgs a)
{
  const uint32_t w = (blockIdx.x * (uint32_t)kBlock + threadIdx.x) >> 6;
  if (w >= (uint32_t)a.group_size * (uint32_t)a.n_labels) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int sl = (int)(w / (uint32_t)a.n_labels), label = (int)(w - (uint32_t)sl * (uint32_t)a.n_labels), stream = a.group_base + sl;
  unsigned long long* row = a.table + ((size_t)stream * (size_t)a.n_labels + (size_t)label) * 2u;
  const unsigned long long key = row[0];
  const uint32_t cnt = (uint32_t)row[1];
  uint32_t cbits = 0x7f800000u, pixel = 0xffffffffu, id = 0xffffffffu;
  if (key != kClearanceNone) {
    cbits = clearance_bits_of_order((uint32_t)(key >> 32));
    pixel = (uint32_t)key;
    const int v = (int)(pixel / (uint32_t)a.width), u = (int)(pixel - (uint32_t)v * (uint32_t)a.width);
    const size_t pix = (size_t)stream * (size_t)a.width * (size_t)a.height + (size_t)pixel;
    const float s = U16 ? u16_to_metres(reinterpret_cast<const uint16_t*>(a.depth)[pix]) : a.depth[pix];
    float px, py, pz;
    cloud_point(u, v, s, a.intr[stream], px, py, pz);
    for (int j = lane; j < a.n_spheres; j += 64) {
      const ClearanceSphere sp = a.spheres[j];
      if (label != 0 && (int)(sp.label_slot & 0xffffu) != label) continue;
      const float4 q = a.posed[(size_t)stream * (size_t)a.n_spheres + (size_t)j];
      if (q.w < 0.0f) continue;
      if (__float_as_uint(clearance_point_sphere(px, py, pz, q.x, q.y, q.z, q.w)) == cbits) id = min(id, sp.id);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) id = min(id, (uint32_t)__shfl_xor((int)id, o));
  }
  if (lane == 0) {
    row[0] = (unsigned long long)cbits | (unsigned long long)pixel << 32;
    row[1] = (unsigned long long)id | (unsigned long long)cnt << 32;
  }
}

void launch_clearance(const ClearanceArgs& a, hipStream_t st)
{
  const size_t rows = (size_t)a.group_size * (size_t)a.n_labels;
  const size_t zblocks = (rows + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(clearance_zero_kernel, dim3((unsigned)(zblocks > 4096 ? 4096 : zblocks)), dim3(kBlock), 0, st,
                     a.table + (size_t)a.group_base * (size_t)a.n_labels * 2u, rows);
  if (a.n_spheres > 0) {
    hipLaunchKernelGGL(clearance_spheres_kernel, dim3((unsigned)((a.n_spheres + kBlock - 1) / kBlock), (unsigned)a.group_size), dim3(kBlock), 0, st, a);
    const size_t waves = (size_t)a.height * (size_t)((a.width + 63) >> 6);
    const dim3 grid((unsigned)((waves + kBlock / 64 - 1) / (kBlock / 64)), (unsigned)a.group_size);
    if (a.io_u16) hipLaunchKernelGGL(clearance_kernel<true>, grid, dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL(clearance_kernel<false>, grid, dim3(kBlock), 0, st, a);
  }
  const unsigned fblocks = (unsigned)((rows * 64u + kBlock - 1) / kBlock);
  if (a.io_u16) hipLaunchKernelGGL(clearance_finish_kernel<true>, dim3(fblocks), dim3(kBlock), 0, st, a);
  else hipLaunchKernelGGL(clearance_finish_kernel<false>, dim3(fblocks), dim3(kBlock), 0, st, a);
}

// ---- scene planes (include/rtuf.h, SCENE PLANES) --------------------------------------------------------------------------
// Two streaming kernels that run behind whatever made a launch group's outputs: they read the sensor plane once more and the
// stream's scene plane, and add the scene's verdict (scene_filtered, rtuf_numerics.h) to outputs that are already complete.
// Neither needs to know why a pixel was filtered before: masked' = scene_filtered ? replace : masked and mask' =
// scene_filtered ? 255 : mask touch filtered pixels only, so nothing of the outputs is read and a masked plane that aliases
// the sensor plane stays legal (a pixel already replaced is rewritten with the same value or left alone).
//
// Shape: a lane takes one 16-byte load of sensor values -- 4 float pixels, 8 16UC1 pixels -- and the matching 16 or 32 bytes of
// the scene plane.  Where all of its pixels are scene-filtered (the common case in a cell with a full scene model: writes are
// dense) it stores 16 bytes of the replace value and 4 or 8 mask bytes in one instruction each; where none is, nothing; only
// the lanes on an object's outline fall back to a store per pixel.  Planes that do not start on 16-byte boundaries (an odd
// image size, a caller's offset pointer) take the one-pixel-per-lane instantiation.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2s __attribute__((ext_vector_type(2)));

// the lane's N sensor values in metres and scene values, from pixel `pix` of the batch / `spix` of the scene planes
template <bool U16, int N>
__device__ __forceinline__ void scene_load(const SceneArgs& a, size_t pix, size_t spix, float (&s)[N], float (&sc)[N])
{
  if constexpr (N == 1) {
    s[0] = U16 ? u16_to_metres(reinterpret_cast<const uint16_t*>(a.depth)[pix]) : a.depth[pix];
    sc[0] = a.scene[spix];
  } else {
    const u32x4 q = *reinterpret_cast<const u32x4*>(U16 ? reinterpret_cast<const char*>(a.depth) + pix * 2u : reinterpret_cast<const char*>(a.depth) + pix * 4u);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (U16) { s[2 * j] = u16_to_metres(w[j] & 0xffffu); s[2 * j + 1] = u16_to_metres(w[j] >> 16); }
      else s[j] = __uint_as_float(w[j]);
    }
#pragma unroll
    for (int k = 0; k < N / 4; k++) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(a.scene + spix + 4 * k);
      sc[4 * k] = v.x; sc[4 * k + 1] = v.y; sc[4 * k + 2] = v.z; sc[4 * k + 3] = v.w;
    }
  }
}

// grid: (ceil(H * W / N / kBlock), group_size)
template <bool U16, bool WIDE>
__global__ __launch_bounds__(kBlock) void scene_apply_planes_kernel(SceneArgs a)
{
  constexpr int N = WIDE ? (U16 ? 8 : 4) : 1;
  const int stream = a.group_base + (int)blockIdx.y;
  const SceneStream ss = a.streams[stream];
  if (!ss.enabled) return;
  const size_t plane = (size_t)a.width * (size_t)a.height;
  const size_t p0 = ((size_t)blockIdx.x * kBlock + threadIdx.x) * (size_t)N;
  if (p0 >= plane) return;                       // (WIDE: N divides the plane)
  const size_t pix = (size_t)stream * plane + p0;
  float s[N], sc[N];
  scene_load<U16, N>(a, pix, pix, s, sc);
  uint32_t f = 0;
#pragma unroll
  for (int j = 0; j < N; j++) f |= (scene_filtered(s[j], sc[j], ss.abs_m, ss.rel) ? 1u : 0u) << j;
  if (!f) return;
  uint16_t* const out16 = reinterpret_cast<uint16_t*>(a.masked) + pix;
  float* const out32 = a.masked + pix;
  const uint32_t rep16 = U16 ? metres_to_u16(a.replace_value) : 0u;
  if (WIDE && f == (1u << N) - 1u) {
    u32x4 o;
    o.x = o.y = o.z = o.w = U16 ? (rep16 | rep16 << 16) : __float_as_uint(a.replace_value);
    __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(U16 ? (void*)out16 : (void*)out32));
    if (a.mask) {
      if (U16) { u32x2s m; m.x = m.y = 0xffffffffu; __builtin_nontemporal_store(m, reinterpret_cast<u32x2s*>(a.mask + pix)); }
      else __builtin_nontemporal_store(0xffffffffu, reinterpret_cast<uint32_t*>(a.mask + pix));
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < N; j++) {
    if (!((f >> j) & 1u)) continue;
    if (U16) out16[j] = (uint16_t)rep16;
    else out32[j] = a.replace_value;
    if (a.mask) a.mask[pix + j] = 255;
  }
}

// The mask-bits form: the lane's N verdicts go to its place in the row's bits word, the 32 / N lanes of a word OR theirs
// together and the first of them ORs the result into the word in place (the only writer of that word; words that gain no bit
// are not written).  grid: (ceil(H * ceil(W/32) * (32 / N) / kBlock), group_size); a word's lanes never straddle a wave.
template <bool U16, bool WIDE>
__global__ __launch_bounds__(kBlock) void scene_apply_bits_kernel(SceneArgs a)
{
  constexpr int N = WIDE ? (U16 ? 8 : 4) : 1;
  constexpr uint32_t kLanesPerWord = 32u / (uint32_t)N;
  const int stream = a.group_base + (int)blockIdx.y;
  const SceneStream ss = a.streams[stream];
  if (!ss.enabled) return;
  const uint32_t row_words = (uint32_t)(a.width + 31) >> 5, row_lanes = row_words * kLanesPerWord;
  const uint32_t t = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  const uint32_t v = t / row_lanes, q = t - v * row_lanes;
  const int u = (int)(q * (uint32_t)N);
  uint32_t f = 0;
  if (v < (uint32_t)a.height && u < a.width) {        // (WIDE: N divides W, the lane's pixels are all inside or all outside)
    const size_t spix = ((size_t)stream * a.height + (size_t)v) * (size_t)a.width + (size_t)u;
    float s[N], sc[N];
    scene_load<U16, N>(a, spix, spix, s, sc);
#pragma unroll
    for (int j = 0; j < N; j++) f |= (scene_filtered(s[j], sc[j], ss.abs_m, ss.rel) ? 1u : 0u) << j;
  }
  uint32_t word = f << ((q & (kLanesPerWord - 1u)) * (uint32_t)N);
#pragma unroll
  for (uint32_t o = 1; o < kLanesPerWord; o <<= 1) word |= (uint32_t)__shfl_xor((int)word, (int)o);
  if ((q & (kLanesPerWord - 1u)) == 0u && word && v < (uint32_t)a.height) {
    uint32_t* const p = a.bits + ((size_t)stream * a.height + (size_t)v) * (size_t)row_words + (size_t)(q / kLanesPerWord);
    const uint32_t old = *p;
    if ((old | word) != old) *p = old | word;
  }
}

void launch_scene_apply(const SceneArgs& a, hipStream_t st)
{
  const int n = a.wide ? (a.io_u16 ? 8 : 4) : 1;
  if (a.bits) {
    const size_t lanes = (size_t)a.height * (size_t)((a.width + 31) >> 5) * (size_t)(32 / n);
    const dim3 grid((unsigned)((lanes + kBlock - 1) / kBlock), (unsigned)a.group_size);
    if (a.wide) {
      if (a.io_u16) hipLaunchKernelGGL((scene_apply_bits_kernel<true, true>), grid, dim3(kBlock), 0, st, a);
      else hipLaunchKernelGGL((scene_apply_bits_kernel<false, true>), grid, dim3(kBlock), 0, st, a);
    } else if (a.io_u16) hipLaunchKernelGGL((scene_apply_bits_kernel<true, false>), grid, dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((scene_apply_bits_kernel<false, false>), grid, dim3(kBlock), 0, st, a);
    return;
  }
  const size_t lanes = ((size_t)a.width * (size_t)a.height + (size_t)n - 1) / (size_t)n;
  const dim3 grid((unsigned)((lanes + kBlock - 1) / kBlock), (unsigned)a.group_size);
  if (a.wide) {
    if (a.io_u16) hipLaunchKernelGGL((scene_apply_planes_kernel<true, true>), grid, dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((scene_apply_planes_kernel<false, true>), grid, dim3(kBlock), 0, st, a);
  } else if (a.io_u16) hipLaunchKernelGGL((scene_apply_planes_kernel<true, false>), grid, dim3(kBlock), 0, st, a);
  else hipLaunchKernelGGL((scene_apply_planes_kernel<false, false>), grid, dim3(kBlock), 0, st, a);
}

// Learning (rtuf_learn_scene_batch*): a pixel per lane, the calibration phase's kernel.  The bits are the robot's alone and
// final (the mask-bits batch that made them has been retired, re-runs included).  grid: (ceil(H * W / kBlock), n).
template <bool U16>
__global__ __launch_bounds__(kBlock) void scene_learn_kernel(SceneLearnArgs a)
{
  const size_t plane = (size_t)a.width * (size_t)a.height;
  const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= plane) return;
  const int stream = (int)blockIdx.y;
  const int v = (int)(p / (size_t)a.width), u = (int)(p - (size_t)v * (size_t)a.width);
  const size_t pix = (size_t)stream * plane + p;
  const float s = U16 ? u16_to_metres(reinterpret_cast<const uint16_t*>(a.depth)[pix]) : a.depth[pix];
  const uint32_t w = a.bits[((size_t)stream * a.height + (size_t)v) * (size_t)((a.width + 31) >> 5) + (size_t)(u >> 5)];
  const float have = a.scene[pix];
  const float next = scene_learned(have, s, ((w >> (u & 31)) & 1u) != 0u);
  if (__float_as_uint(next) != __float_as_uint(have)) a.scene[pix] = next;
}
void launch_scene_learn(const SceneLearnArgs& a, hipStream_t st)
{
  const dim3 grid((unsigned)(((size_t)a.width * a.height + kBlock - 1) / kBlock), (unsigned)a.n_streams);
  if (a.io_u16) hipLaunchKernelGGL(scene_learn_kernel<true>, grid, dim3(kBlock), 0, st, a);
  else hipLaunchKernelGGL(scene_learn_kernel<false>, grid, dim3(kBlock), 0, st, a);
}

// ---- point list batches (include/rtuf.h, POINT LIST BATCHES) -------------------------------------------------------------
// Behind the launch group's tile_render_kernel on its lane: every point of every stream of the group is projected into its
// stream's virtual depth plane (point_pixel), compared with the smallest value of its window there (point_verdict) and given
// a verdict byte.  A latency-bound gather: a thread takes kPointsPerThread consecutive points of one stream, so their window
// loads are in flight together, a wave's point loads are contiguous 12-byte triples (three 16-byte loads per thread on the
// wide path) and the verdicts leave as words.  Integers only in the summary: no result depends on the order of execution.
// grid: (ceil(capacity / (kBlock * kPointsPerThread)), group_size).

__global__ __launch_bounds__(kBlock) void points_zero_summary_kernel(uint32_t* rows, int n_words)
{
  const int i = (int)(blockIdx.x * (uint32_t)kBlock + threadIdx.x);
  if (i < n_words) rows[i] = 0u;
}

// The smallest value of the (2R + 1)^2 window around (u, v), its rows and columns clamped to the stream's image -- never padded,
// never in a neighbouring plane; a clamped index reads a pixel of the window a second time, which no minimum notices.  The
// radius is a template argument so that a row's 2R + 1 loads are issued together.
template <int R>
__device__ __forceinline__ float points_window_min(const float* __restrict__ plane, int u, int v, int width, int height)
{
  float vmin = INFINITY;
#pragma unroll 1
  for (int dy = -R; dy <= R; dy++) {
    const float* row = plane + (size_t)min(max(v + dy, 0), height - 1) * (size_t)width;
    float q[2 * R + 1];
#pragma unroll
    for (int dx = -R; dx <= R; dx++) q[dx + R] = row[min(max(u + dx, 0), width - 1)];
#pragma unroll
    for (int dx = 0; dx <= 2 * R; dx++) vmin = fminf(vmin, q[dx]);
  }
  return vmin;
}

template <int R>
__global__ __launch_bounds__(kBlock) void points_filter_kernel(PointsArgs a)
{
  const int stream = a.group_base + (int)blockIdx.y;
  const uint32_t capacity = (uint32_t)a.capacity;
  const uint32_t have = a.counts[stream];
  const uint32_t m = have < capacity ? have : capacity;
  if (a.summary && blockIdx.x == 0 && threadIdx.x == 0) a.summary[(size_t)stream * 4u + 3u] = m;
  const uint32_t t = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  const uint32_t j0 = t * (uint32_t)kPointsPerThread;
  // (wave-uniform: the wave's first point is its lane 0's; lanes past m stay for the ballots and load nothing)
  if ((j0 & ~(64u * (uint32_t)kPointsPerThread - 1u)) >= m) return;
  const size_t base = (size_t)stream * (size_t)capacity + (size_t)j0;
  const uint32_t live = j0 >= m ? 0u : (m - j0 < (uint32_t)kPointsPerThread ? m - j0 : (uint32_t)kPointsPerThread);
  const bool whole = a.wide && live == (uint32_t)kPointsPerThread;
  float p[3 * kPointsPerThread];
  if (whole) {
    const float4* src = reinterpret_cast<const float4*>(a.points + base * 3u);
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const float4 q = src[i];
      p[4 * i] = q.x; p[4 * i + 1] = q.y; p[4 * i + 2] = q.z; p[4 * i + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 3 * kPointsPerThread; i++) p[i] = (uint32_t)(i / 3) < live ? a.points[base * 3u + (size_t)i] : 0.0f;
  }
  const PointIntrinsics k = a.intr[stream];
  const PointTransform* tf = a.tf + stream;
  const bool moved = tf->on != 0u;
  const float* plane = a.virt + (size_t)stream * (size_t)a.width * (size_t)a.height;
  uint32_t verdict[kPointsPerThread], pixel[kPointsPerThread];
#pragma unroll
  for (int i = 0; i < kPointsPerThread; i++) {
    float x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
    if (moved) point_transform(tf->m, x, y, z);
    int u, v;
    verdict[i] = kPointOutside;
    pixel[i] = kPointNoPixel;
    if ((uint32_t)i < live && point_pixel(x, y, z, k, a.width, a.height, u, v)) {
      verdict[i] = point_verdict(z, points_window_min<R>(plane, u, v, a.width, a.height), a.threshold);
      pixel[i] = (uint32_t)(v * a.width + u);
    }
  }
  if (whole) {
    *reinterpret_cast<uint32_t*>(a.verdict + base) = verdict[0] | verdict[1] << 8 | verdict[2] << 16 | verdict[3] << 24;
    if (a.pixel) *reinterpret_cast<uint4*>(a.pixel + base) = make_uint4(pixel[0], pixel[1], pixel[2], pixel[3]);
  } else {
#pragma unroll
    for (int i = 0; i < kPointsPerThread; i++)
      if ((uint32_t)i < live) {
        a.verdict[base + (size_t)i] = (uint8_t)verdict[i];
        if (a.pixel) a.pixel[base + (size_t)i] = pixel[i];
      }
  }
  if (a.summary) {
    // per wave and class: the ballots of the lanes' points, one vector atomic from the wave's first lane
    uint32_t total[3] = {0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < kPointsPerThread; i++)
#pragma unroll
      for (uint32_t c = 0; c < 3u; c++) total[c] += (uint32_t)__popcll(__ballot((uint32_t)i < live && verdict[i] == c));
    if ((threadIdx.x & 63u) == 0u)
#pragma unroll
      for (int c = 0; c < 3; c++)
        if (total[c]) atomicAdd(a.summary + (size_t)stream * 4u + (size_t)c, total[c]);
  }
}
static_assert(kPointsPerThread == 4, "points_filter_kernel packs four verdicts into a word and four pixels into a 16-byte store");

void launch_points(const PointsArgs& a, hipStream_t st)
{
  if (a.summary) {
    const int n_words = a.group_size * 4;
    hipLaunchKernelGGL(points_zero_summary_kernel, dim3((unsigned)((n_words + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       a.summary + (size_t)a.group_base * 4u, n_words);
  }
  const unsigned per_block = (unsigned)kBlock * (unsigned)kPointsPerThread;
  const dim3 grid(((unsigned)a.capacity + per_block - 1u) / per_block, (unsigned)a.group_size);
  switch (a.radius) {      // (0 .. kMaxPointsRadius: the call's checks admit nothing else)
    case 0: hipLaunchKernelGGL(points_filter_kernel<0>, grid, dim3(kBlock), 0, st, a); break;
    case 1: hipLaunchKernelGGL(points_filter_kernel<1>, grid, dim3(kBlock), 0, st, a); break;
    case 2: hipLaunchKernelGGL(points_filter_kernel<2>, grid, dim3(kBlock), 0, st, a); break;
    case 3: hipLaunchKernelGGL(points_filter_kernel<3>, grid, dim3(kBlock), 0, st, a); break;
    case 4: hipLaunchKernelGGL(points_filter_kernel<4>, grid, dim3(kBlock), 0, st, a); break;
    default: break;
  }
  static_assert(kMaxPointsRadius == 4, "launch_points names an instantiation per radius");
}

// ---- voxel occupancy grids (include/rtuf.h, VOXEL OCCUPANCY GRIDS) ---------------------------------------------------------
// One insert: every kept pixel (plane form) or taken list entry (list form) of every stream becomes a world point
// (cloud_point, point_transform), the point a voxel index (voxel_of), and the voxel gets its bit ORed and its count added.
// Neighbouring pixels mostly share a voxel -- a 5 cm voxel at 1 m is 25 VGA pixels wide -- so one atomic per pixel would
// serialise on a few addresses of a grid all XCDs share.  A thread holds four consecutive pixels (entries): equal neighbours
// are merged inside the thread first, then runs of equal index across adjacent lanes of the wave, and the run's first lane
// issues one atomicOr and one atomicAdd for the whole run (relaxed, agent scope).  Lane order is pixel order, a row's end next
// to the following row's start: a run may cross rows, its sum is the same.  Integers only: no result depends on the order
// of execution.

__global__ __launch_bounds__(kBlock) void voxel_clear_kernel(uint4* p, size_t n16)
{
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n16; i += (size_t)gridDim.x * kBlock) p[i] = make_uint4(0u, 0u, 0u, 0u);
}
void launch_voxel_clear(uint32_t* p, size_t n_words, hipStream_t st)
{
  const size_t n16 = n_words / 4u, blocks = (n16 + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(voxel_clear_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks))), dim3(kBlock), 0, st, reinterpret_cast<uint4*>(p), n16);
}

// n points in voxel idx (voxel_of's index: below the grid's size, or kVoxelNone: nothing to do)
__device__ __forceinline__ void voxel_emit(const VoxelArgs& a, uint32_t idx, uint32_t n)
{
  if (idx == kVoxelNone) return;
  __hip_atomic_fetch_or(a.grid_bits + (idx >> 5), 1u << (idx & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (a.grid_counts) __hip_atomic_fetch_add(a.grid_counts + idx, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The four indices of every lane of the wave, in lane order (every lane of the wave calls this, lanes without work with four
// kVoxelNone).  A lane's HEAD run holds its entry 0 and what equals it behind, its TAIL run its entry 3 and what equals it in
// front; a UNIFORM lane is one run of four.  Entries 1 and 2 outside both runs are emitted by the lane itself.  A lane JOINS
// when its entry 0 equals the previous lane's entry 3: its head run is then part of the chain that previous lane's tail run
// belongs to, and a uniform lane that joins passes the chain on.  Every other tail run starts a chain: its lane adds the 4s of
// the uniform joining lanes behind it and the head run of the lane that ends the chain, and emits once.
__device__ __forceinline__ void voxel_aggregate(const VoxelArgs& a, const uint32_t (&idx)[4])
{
  const uint32_t lane = threadIdx.x & 63u;
  const bool uniform = idx[0] == idx[1] && idx[1] == idx[2] && idx[2] == idx[3];
  const uint32_t ch = idx[1] != idx[0] ? 1u : (idx[2] != idx[0] ? 2u : 3u);                   // (of a lane that is not uniform: 1 .. 3)
  const uint32_t ct = uniform ? 4u : (idx[2] != idx[3] ? 1u : (idx[1] != idx[3] ? 2u : 3u));
  const bool in1 = !uniform && ch == 1u && ct <= 2u, in2 = !uniform && ct == 1u && ch <= 2u;  // entries 1, 2 in neither run
  if (in1 && in2 && idx[1] == idx[2]) voxel_emit(a, idx[1], 2u);
  else {
    if (in1) voxel_emit(a, idx[1], 1u);
    if (in2) voxel_emit(a, idx[2], 1u);
  }
  const uint32_t prev_tail = __shfl_up(idx[3], 1);
  const bool joins = lane > 0u && idx[0] == prev_tail;
  const unsigned long long J = __ballot(joins), C = __ballot(joins && uniform);
  const unsigned long long stop = ((~C) >> 1) >> lane;              // bit i: lane + 1 + i does not pass a chain on
  const uint32_t m = stop ? lane + 1u + (uint32_t)__builtin_ctzll(stop) : 64u;      // the chain's last lane, if it joins; 64: the wave ends first
  const uint32_t ch_m = __shfl(ch, (int)(m & 63u));
  if (!(joins && uniform)) voxel_emit(a, idx[3], ct + 4u * (m - lane - 1u) + (m < 64u && ((J >> m) & 1ull) ? ch_m : 0u));
  if (!uniform && !joins) voxel_emit(a, idx[0], ch);
}

// The summary's three counted fields of one stream (row: its four words, zeroed in front of the kernel): per wave a packed
// add-reduction (at most 4 per lane and field: 256 per wave, 10-bit fields), per workgroup in LDS, then one atomic per
// workgroup and field.  Every thread of the workgroup calls this.
__device__ __forceinline__ void voxel_summarise(uint32_t* row, uint32_t inserted, uint32_t outside, uint32_t not_kept)
{
  __shared__ uint32_t total[3];
  if (threadIdx.x < 3u) total[threadIdx.x] = 0u;
  __syncthreads();
  uint32_t w = inserted | outside << 10 | not_kept << 20;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) w += (uint32_t)__shfl_xor((int)w, o);
  if ((threadIdx.x & 63u) == 0u && w) {
    if (w & 1023u) atomicAdd(&total[0], w & 1023u);
    if ((w >> 10) & 1023u) atomicAdd(&total[1], (w >> 10) & 1023u);
    if (w >> 20) atomicAdd(&total[2], w >> 20);
  }
  __syncthreads();
  if (threadIdx.x < 3u && total[threadIdx.x]) atomicAdd(row + threadIdx.x, total[threadIdx.x]);
}

// Plane form: one thread per four consecutive pixels of a row -- one 16-byte (f32) or 8-byte (16UC1) sensor load on the wide
// path, scalar loads otherwise (a row's remainder when W % 4 != 0 included), and the pixels' nibble of their bits word.  The
// stream is the workgroup's (blockIdx.y): intrinsics, matrix and grid are read through uniform addresses.
// grid: (ceil(H * ceil(W / 4) / kBlock), n).
template <bool U16>
__global__ __launch_bounds__(kBlock) void voxel_insert_kernel(VoxelArgs a)
{
  const int stream = (int)blockIdx.y;
  const int w4 = (a.width + 3) >> 2;
  const uint32_t t = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  uint32_t idx[4] = {kVoxelNone, kVoxelNone, kVoxelNone, kVoxelNone};
  uint32_t inserted = 0u, outside = 0u, not_kept = 0u;
  if (t < (uint32_t)w4 * (uint32_t)a.height) {
    const int v = (int)(t / (uint32_t)w4), u = (int)(t - (uint32_t)v * (uint32_t)w4) * 4;
    const int nvalid = a.width - u < 4 ? a.width - u : 4;
    const size_t pix = ((size_t)stream * (size_t)a.height + (size_t)v) * (size_t)a.width + (size_t)u;
    float s[4];
    if (a.wide) {
      if (U16) {
        const uint2 q = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(a.depth) + pix);
        s[0] = u16_to_metres(q.x & 0xffffu); s[1] = u16_to_metres(q.x >> 16); s[2] = u16_to_metres(q.y & 0xffffu); s[3] = u16_to_metres(q.y >> 16);
      } else {
        const float4 q = *reinterpret_cast<const float4*>(a.depth + pix);
        s[0] = q.x; s[1] = q.y; s[2] = q.z; s[3] = q.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        s[j] = j < nvalid ? (U16 ? u16_to_metres(reinterpret_cast<const uint16_t*>(a.depth)[pix + (size_t)j]) : a.depth[pix + (size_t)j]) : 0.0f;
    }
    const int row_words = (a.width + 31) >> 5;
    const uint32_t nib = a.bits[((size_t)stream * a.height + (size_t)v) * (size_t)row_words + (size_t)(u >> 5)] >> (u & 31);
    const CloudIntrinsics k = a.intr[stream];
    const VoxelGrid g = {a.ox, a.oy, a.oz, a.inv, a.nx, a.ny, a.nz};
    const PointTransform* tf = a.world_tf ? a.world_tf + stream : nullptr;
    const bool moved = tf && tf->on != 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (j >= nvalid) continue;
      if (((nib >> j) & 1u) || !cloud_sensor_valid(s[j])) { not_kept++; continue; }
      float x, y, z;
      cloud_point(u + j, v, s[j], k, x, y, z);
      if (moved) point_transform(tf->m, x, y, z);
      if (voxel_of(x, y, z, g, idx[j])) inserted++;
      else outside++;
    }
  }
  voxel_aggregate(a, idx);
  if (a.summary) {
    if (blockIdx.x == 0u && threadIdx.x == 0u) a.summary[(size_t)stream * 4u + 3u] = (uint32_t)a.width * (uint32_t)a.height;
    voxel_summarise(a.summary + (size_t)stream * 4u, inserted, outside, not_kept);
  }
}

// List form: a thread takes kPointsPerThread consecutive entries of one stream, as points_filter_kernel does (three 16-byte
// loads and the verdicts' word on the wide path).  grid: (ceil(capacity / (kBlock * kPointsPerThread)), n).
__global__ __launch_bounds__(kBlock) void voxel_insert_points_kernel(VoxelArgs a)
{
  const int stream = (int)blockIdx.y;
  const uint32_t capacity = (uint32_t)a.capacity;
  const uint32_t have = a.counts[stream];
  const uint32_t m = have < capacity ? have : capacity;
  const uint32_t t = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  const uint32_t j0 = t * (uint32_t)kPointsPerThread;
  const uint32_t live = j0 >= m ? 0u : (m - j0 < (uint32_t)kPointsPerThread ? m - j0 : (uint32_t)kPointsPerThread);
  uint32_t idx[4] = {kVoxelNone, kVoxelNone, kVoxelNone, kVoxelNone};
  uint32_t inserted = 0u, outside = 0u, not_kept = 0u;
  if (live) {
    const size_t base = (size_t)stream * (size_t)capacity + (size_t)j0;
    float p[3 * kPointsPerThread];
    uint32_t verdict[kPointsPerThread] = {0u, 0u, 0u, 0u};
    if (a.wide && live == (uint32_t)kPointsPerThread) {
      const float4* src = reinterpret_cast<const float4*>(a.points + base * 3u);
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const float4 q = src[i];
        p[4 * i] = q.x; p[4 * i + 1] = q.y; p[4 * i + 2] = q.z; p[4 * i + 3] = q.w;
      }
      if (a.verdict) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(a.verdict + base);
#pragma unroll
        for (int i = 0; i < kPointsPerThread; i++) verdict[i] = (w >> (8 * i)) & 255u;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 3 * kPointsPerThread; i++) p[i] = (uint32_t)(i / 3) < live ? a.points[base * 3u + (size_t)i] : 0.0f;
      if (a.verdict)
#pragma unroll
        for (int i = 0; i < kPointsPerThread; i++) verdict[i] = (uint32_t)i < live ? (uint32_t)a.verdict[base + (size_t)i] : 0u;
    }
    const VoxelGrid g = {a.ox, a.oy, a.oz, a.inv, a.nx, a.ny, a.nz};
    const PointTransform* ptf = a.point_tf ? a.point_tf + stream : nullptr;
    const PointTransform* wtf = a.world_tf ? a.world_tf + stream : nullptr;
    const bool moved = ptf && ptf->on != 0u, moved_again = wtf && wtf->on != 0u;
#pragma unroll
    for (int i = 0; i < kPointsPerThread; i++) {
      if ((uint32_t)i >= live) continue;
      if (verdict[i] != kPointKept) { not_kept++; continue; }
      float x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
      if (moved) point_transform(ptf->m, x, y, z);
      if (moved_again) point_transform(wtf->m, x, y, z);
      if (voxel_of(x, y, z, g, idx[i])) inserted++;
      else outside++;
    }
  }
  voxel_aggregate(a, idx);
  if (a.summary) {
    if (blockIdx.x == 0u && threadIdx.x == 0u) a.summary[(size_t)stream * 4u + 3u] = m;
    voxel_summarise(a.summary + (size_t)stream * 4u, inserted, outside, not_kept);
  }
}
static_assert(kPointsPerThread == 4, "voxel_aggregate merges four entries per lane");

void launch_voxel_insert(const VoxelArgs& a, hipStream_t st)
{
  if (a.summary) {
    const int n_words = a.n_streams * 4;
    hipLaunchKernelGGL(points_zero_summary_kernel, dim3((unsigned)((n_words + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a.summary, n_words);
  }
  if (a.points) {
    const unsigned per_block = (unsigned)kBlock * (unsigned)kPointsPerThread;
    hipLaunchKernelGGL(voxel_insert_points_kernel, dim3(((unsigned)a.capacity + per_block - 1u) / per_block, (unsigned)a.n_streams), dim3(kBlock), 0, st, a);
    return;
  }
  const size_t lanes = (size_t)a.height * (size_t)((a.width + 3) >> 2);
  const dim3 grid((unsigned)((lanes + kBlock - 1) / kBlock), (unsigned)a.n_streams);
  if (a.io_u16) hipLaunchKernelGGL(voxel_insert_kernel<true>, grid, dim3(kBlock), 0, st, a);
  else hipLaunchKernelGGL(voxel_insert_kernel<false>, grid, dim3(kBlock), 0, st, a);
}

// ---- voxel free space (include/rtuf.h, VOXEL FREE SPACE) -------------------------------------------------------------------
// One carve, projectively: a thread owns one voxel, consecutive lanes consecutive indices (they run along x, so a wave's
// gathers fall on neighbouring pixels), and walks the streams: centre (voxel_centre) -> optical frame (point_transform with
// the stream's inverse) -> pixel (point_pixel) -> the sensor value there and, with a radius, the smallest valid value of its
// window -> voxel_free_test.  The stream's two records are read through uniform addresses.  A wave none of whose lanes is
// judged by a stream issues no gather for it.  At the end one 64-bit ballot is the wave's two output words: lane 0 reads, ORs
// and writes them with ordinary 8-byte accesses -- one owner per word, no atomics on the grid; lanes past n_voxels are never
// free, so the last word's upper bits stay 0.  SUMMARY: per (wave, stream) the popcounts of two ballots go into a table of the
// workgroup in LDS, flushed with one atomic per workgroup, stream and field for every kCarveChunk streams; "not seen" and the
// total are filled in behind the kernel (voxel_carve_finish_kernel).  Without a summary a lane that is free stops gathering
// and a wave whose live lanes are all free leaves the loop: the bits are the same.
constexpr int kCarveChunk = 256;

template <bool U16>
__device__ __forceinline__ float carve_sensor(const float* __restrict__ plane, size_t i)
{
  return U16 ? u16_to_metres(reinterpret_cast<const uint16_t*>(plane)[i]) : plane[i];
}

template <bool U16, bool SUMMARY>
__global__ __launch_bounds__(kBlock) void voxel_carve_kernel(VoxelCarveArgs a)
{
  __shared__ uint32_t tab[SUMMARY ? 2 * kCarveChunk : 1];
  const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  const bool live = i < a.n_voxels;
  const uint32_t lane = threadIdx.x & 63u;
  float wx = 0.0f, wy = 0.0f, wz = 0.0f;
  if (live) {
    const uint32_t row = i / (uint32_t)a.nx, ix = i - row * (uint32_t)a.nx;
    const uint32_t iz = row / (uint32_t)a.ny, iy = row - iz * (uint32_t)a.ny;
    wx = voxel_centre((int)ix, a.ox, a.size);
    wy = voxel_centre((int)iy, a.oy, a.size);
    wz = voxel_centre((int)iz, a.oz, a.size);
  }
  const size_t plane_px = (size_t)a.width * (size_t)a.height;
  bool free_any = false;
  for (int s0 = 0; s0 < a.n_streams; s0 += kCarveChunk) {
    const int s1 = min(s0 + kCarveChunk, a.n_streams);
    if (SUMMARY) {
      for (int j = (int)threadIdx.x; j < 2 * (s1 - s0); j += kBlock) tab[j] = 0u;
      __syncthreads();
    }
    for (int s = s0; s < s1; s++) {
      if (!SUMMARY && __ballot(live && !free_any) == 0ull) break;
      float x = wx, y = wy, z = wz;
      if (a.inv_tf && a.inv_tf[s].on != 0u) point_transform(a.inv_tf[s].m, x, y, z);
      const PointIntrinsics k = a.intr[s];
      int u, v;
      const bool judged = live && point_pixel(x, y, z, k, a.width, a.height, u, v);
      bool free_here = false;
      if (judged && (SUMMARY || !free_any)) {      // (a wave without such a lane branches round the gathers)
        const float* __restrict__ plane = U16 ? reinterpret_cast<const float*>(reinterpret_cast<const uint16_t*>(a.depth) + (size_t)s * plane_px)
                                              : a.depth + (size_t)s * plane_px;
        const float centre = carve_sensor<U16>(plane, (size_t)v * (size_t)a.width + (size_t)u);
        if (cloud_sensor_valid(centre)) {
          float emin = centre;
          if (a.radius > 0) {
            const int v0 = max(v - a.radius, 0), v1 = min(v + a.radius, a.height - 1);
            const int u0 = max(u - a.radius, 0), u1 = min(u + a.radius, a.width - 1);
            for (int vv = v0; vv <= v1; vv++)
              for (int uu = u0; uu <= u1; uu++) {
                const float q = carve_sensor<U16>(plane, (size_t)vv * (size_t)a.width + (size_t)uu);
                if (cloud_sensor_valid(q)) emin = fminf(emin, q);
              }
          }
          free_here = voxel_free_test(z, emin, a.margin);
        }
      }
      free_any = free_any || free_here;
      if (SUMMARY) {
        const unsigned long long bf = __ballot(free_here), bn = __ballot(judged && !free_here);
        if (lane == 0u) {
          if (bf) atomicAdd(&tab[2 * (s - s0)], (uint32_t)__popcll(bf));
          if (bn) atomicAdd(&tab[2 * (s - s0) + 1], (uint32_t)__popcll(bn));
        }
      }
    }
    if (SUMMARY) {
      __syncthreads();
      for (int j = (int)threadIdx.x; j < 2 * (s1 - s0); j += kBlock)
        if (tab[j]) atomicAdd(a.summary + (size_t)(s0 + (j >> 1)) * 4u + (size_t)(j & 1), tab[j]);
      __syncthreads();
    }
  }
  const unsigned long long word = __ballot(free_any);
  if (lane == 0u && word != 0ull) {
    // (i is a multiple of 64 here: words i / 32 and i / 32 + 1, inside the array's multiple of four words)
    uint2* const p = reinterpret_cast<uint2*>(a.free_bits + (i >> 5));
    uint2 w = *p;
    w.x |= (uint32_t)word; w.y |= (uint32_t)(word >> 32);
    *p = w;
  }
}

// rows [n][4] hold free and not free: not seen = n_voxels - free - not free, total = n_voxels
__global__ __launch_bounds__(kBlock) void voxel_carve_finish_kernel(uint32_t* rows, int n, uint32_t n_voxels)
{
  const int s = (int)(blockIdx.x * (uint32_t)kBlock + threadIdx.x);
  if (s >= n) return;
  rows[4 * s + 2] = n_voxels - rows[4 * s] - rows[4 * s + 1];
  rows[4 * s + 3] = n_voxels;
}

void launch_voxel_carve(const VoxelCarveArgs& a, hipStream_t st)
{
  const dim3 grid((a.n_voxels + (uint32_t)kBlock - 1u) / (uint32_t)kBlock);
  if (a.summary) {
    const int n_words = a.n_streams * 4;
    hipLaunchKernelGGL(points_zero_summary_kernel, dim3((unsigned)((n_words + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a.summary, n_words);
    if (a.io_u16) hipLaunchKernelGGL((voxel_carve_kernel<true, true>), grid, dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((voxel_carve_kernel<false, true>), grid, dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(voxel_carve_finish_kernel, dim3((unsigned)((a.n_streams + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a.summary, a.n_streams, a.n_voxels);
    return;
  }
  if (a.io_u16) hipLaunchKernelGGL((voxel_carve_kernel<true, false>), grid, dim3(kBlock), 0, st, a);
  else hipLaunchKernelGGL((voxel_carve_kernel<false, false>), grid, dim3(kBlock), 0, st, a);
}

__global__ __launch_bounds__(kBlock) void fill_f32_kernel(float* p, size_t n, float v)
{
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) p[i] = v;
}
void launch_fill_f32(float* p, size_t n, float v, hipStream_t st)
{
  const size_t blocks = (n + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(fill_f32_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks))), dim3(kBlock), 0, st, p, n, v);
}

}  // namespace rtuf
