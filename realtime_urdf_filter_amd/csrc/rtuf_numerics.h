// rtuf_numerics.h -- the arithmetic whose exact bits the results depend on and that something besides the kernels checks or
// shares: the 24-bit depth and its bit-pattern forms, the depth keys' encoding of a near fragment's float z, the set-up's
// 32-bit edge constants, the key format's host-side rules, the compare threshold's constants, division core and the rule
// that admits that core, the pixel classes of the link residual tables, the point of a filtered point cloud, the pixel and
// verdict of a listed point, the voxel of a world point, a voxel's centre, inverse transform and free test, the sphere centres and point-to-sphere clearances of the link clearance tables, the reach of a
// padded link's pixel, the scene planes' threshold and learning rule, and the set-up kernel's packed list counters.
//
// Included by the kernels (rtuf_kernels.hip, device and host pass), the host API (rtuf_api.cpp), scripts/fdiv_check.hip (which
// holds div_core against the IEEE division on the GPU) and the CPU checks (tests/fast_class_check.cpp, tests/near_key_check.cpp:
// plain g++, no ROCm headers), which hold every function here against a reference form of their own.  Every function has ONE
// body, written with the HIP intrinsics the kernels use; only where HIP is absent (the CPU checks) does this file define the
// handful of them it needs, as portable forms with the same results.  No product here feeds an addition -- except in the link clearance
// functions at the end, which say so: their includers compile with -ffp-contract=off (the library, tests/clearance_check.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>

#ifdef __HIP__
#include <hip/hip_runtime.h>
#define RTUF_NUMERIC __device__ __forceinline__
#define RTUF_NUMERIC_HD __host__ __device__ __forceinline__
#else
#define RTUF_NUMERIC inline
#define RTUF_NUMERIC_HD inline
#endif

namespace rtuf {

#ifndef __HIP__
// Without HIP: the intrinsics used below, with the same results.  (The bodies call the intrinsics by name, not through wrappers
// of our own: a wrapper around __mul24 alone changes the instruction schedule of the tile kernel.)
inline float __fmul_rn(float a, float b) { return a * b; }
inline float __fadd_rn(float a, float b) { return a + b; }
inline float __fsub_rn(float a, float b) { return a - b; }
inline float __fdiv_rn(float a, float b) { return a / b; }
inline int __float2int_rn(float x)      // (round half to even: the default rounding mode; saturating, NaN -> 0: v_cvt_i32_f32)
{
  if (!(x == x)) return 0;
  if (x >= 2147483648.0f) return 2147483647;
  if (x <= -2147483648.0f) return -2147483647 - 1;
  return (int)rintf(x);
}
inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
inline int __mul24(int a, int b)      // v_mul_i32_i24: the low 32 bits of the product of the sign-extended low 24 bits
{
  const int64_t x = (int32_t)((uint32_t)a << 8) >> 8, y = (int32_t)((uint32_t)b << 8) >> 8;
  return (int)(uint32_t)(uint64_t)(x * y);
}
#endif

// ---------------------------------------------------------------------------------------
// depths
// ---------------------------------------------------------------------------------------

// 24-bit depth-buffer value of a window z: round(clamp(z, 0, 1) * (2^24 - 1)), half to even (llvmpipe Z24)
RTUF_NUMERIC uint32_t z24_of(float z)
{
  const float zc = fminf(fmaxf(z, 0.0f), 1.0f);
  return (uint32_t)__float2int_rn(__fmul_rn(zc, 16777215.0f));
}

// 24-bit depth of a window z that is KNOWN to be above 0.5 (tiles without near geometry: every record and fragment there has
// z >= 0.51 over its whole box, that is what kNearBit / the bin's near flag say): p = clamp(z) * 16777215 then lies in
// [2^23, 2^24), where a float IS an integer (ulp 1: the product's rounding is the rounding to integer, half to even, that
// v_rndne_f32 would repeat), and its bit pattern is 0x4B000000 + (p - 2^23): one integer add instead of v_rndne + v_cvt.
// (Equal to z24_of for every float z > 0.5: tests/fast_class_check.cpp.)
RTUF_NUMERIC uint32_t z24_of_upper_half(float z)
{
  const float zc = fminf(fmaxf(z, 0.0f), 1.0f);
  return __float_as_uint(__fmul_rn(zc, 16777215.0f)) - 0x4A800000u;
}

// The float z of a winner with 24-bit depth z24 >= 2^23 - 1: (z24 + 1) * 2^-24, whose bit pattern is z24 + 0x3E800001 (the
// integer is its own mantissa, the power of two an exponent offset, and 2^24 carries into the exponent) -- one 2-cycle add
// instead of a conversion and a multiply.  (Every such z24: tests/fast_class_check.cpp.)
RTUF_NUMERIC float z_of_upper_half_z24(uint32_t z24) { return __uint_as_float(z24 + 0x3E800001u); }

// ---------------------------------------------------------------------------------------
// depth keys: {z24, draw order << shift | low `shift` bits of the fragment's float z} (KeyFmt, rtuf_kernels.hip)
// ---------------------------------------------------------------------------------------

// The key's shift for a context of n_tris triangles: draw orders 1 .. n_tris (0 = background quad) take the word's top bits,
// the rest carries the float z's low bits -- at most 16: by then the exact-z pass is needed only within nanometres of the
// near plane.
inline int key_shift_for(uint32_t n_tris)
{
  int order_bits = 1;
  while (((uint64_t)1 << order_bits) <= n_tris) order_bits++;
  return 32 - order_bits < 16 ? 32 - order_bits : 16;
}

// In a tile with near geometry, winners with z24 below this need the exact-z pass: z24 and the float's low `shift` bits pin
// the float down as long as z24's interval of 2^-24 holds fewer than 2^(shift-1) floats, i.e. for z24 >= 2^(26-shift)
// (near_z_from_key).
RTUF_NUMERIC uint32_t exact_z_floor(int shift) { return 1u << (26 - shift); }

// float z of a fragment from its 24-bit depth (exact_z_floor <= z24 <= 2^23) and the low `shift` bits of its float
// (every such float, every shift key_shift_for returns: tests/near_key_check.cpp)
RTUF_NUMERIC float near_z_from_key(uint32_t z24, uint32_t low, int shift)
{
  const uint32_t cb = __float_as_uint(__fmul_rn((float)z24, 5.9604648328104515e-08f));      // about the middle of z24's interval
  const uint32_t span = 1u << shift;
  uint32_t cand = (cb & ~(span - 1u)) | low;
  const int d = (int)(cand - cb);
  const int half = (int)(span >> 1);
  cand = d > half ? cand - span : (d < -half ? cand + span : cand);
  return __uint_as_float(cand);
}

// ---------------------------------------------------------------------------------------
// edge functions of a snapped triangle (1/256 px): inside <=> A px + B py + C > 0, A = -dcdx, B = dcdy
// ---------------------------------------------------------------------------------------

// Inclusive on low-x / low-row edges: dcdx < 0 || (dcdx == 0 && dcdy > 0)  <=>  2 dcdx - (dcdy > 0) < 0, as shifts and
// subtractions (2-cycle instructions instead of compares and selects).
RTUF_NUMERIC uint32_t inclusive_edge_bias(int dcdx, int dcdy) { return ((uint32_t)(dcdx + dcdx) - ((uint32_t)(0 - dcdy) >> 31)) >> 31; }

// C = ceil((dcdx x - dcdy y + bias) / 256) for the edge from vertex (x, y), without 64-bit arithmetic (two 24-bit multiplies
// with their high halves, four carry operations, a 64-bit shift and a branch for the bias, all in the 4-cycle class): with
// x = 256 X + xf, y = 256 Y + yf
//   c = 256 (dcdx X - dcdy Y) + t,   t = dcdx xf - dcdy yf + bias   (|t| < 2^29: exact in 32 bits)
//   ceil(c / 256) = (dcdx X - dcdy Y) + ceil(t / 256)
// and only C's low 32 bits are ever used (the edge value at a pixel of the tile is small; A px + B py + C is evaluated
// modulo 2^32).  (The 64-bit form's low 32 bits for 120 M vertex pairs: tests/fast_class_check.cpp.)
RTUF_NUMERIC int edge_constant(int dcdx, int dcdy, int x, int y)
{
  const int X = x >> 8, Y = y >> 8, xf = x & 255, yf = y & 255;
  const uint32_t bias = inclusive_edge_bias(dcdx, dcdy);
  const int t = __mul24(dcdx, xf) - __mul24(dcdy, yf) + (int)bias;
  return (int)((uint32_t)__mul24(dcdx, X) - (uint32_t)__mul24(dcdy, Y) + (uint32_t)(-((-t) >> 8)));
}

// ---------------------------------------------------------------------------------------
// compare threshold: sensor > num / (z - off) - max_diff  (include/shaders/urdf_filter.frag:14-23)
// ---------------------------------------------------------------------------------------

// to_linear_depth's constants exactly as the shader evaluates them, in float (host only: once per batch)
inline float shade_num(float z_near, float z_far) { return (z_near * z_far) / (z_near - z_far); }
inline float shade_off(float z_near, float z_far) { return z_far / (z_far - z_near); }

// May the per-pixel division num / (z - off) run as div_core?  It needs neither the operand scaling nor the special-case
// fix-up of the IEEE expansion when no operand or intermediate can leave the normal range: |num| within 2^+-40, off in
// [1 + 2^-10, 2^20] (every z the kernels hand to it lies in [-1, 1 + 2^-11]: |z - off| >= 2^-11).  Anything else -- a far
// plane more than a thousand times the near plane, non-finite parameters -- keeps the full expansion.
inline bool fast_div_admitted(float num, float off)
{
  const float a = std::fabs(num);
  return std::isfinite(num) && std::isfinite(off) && a >= 0x1p-40f && a <= 0x1p40f && off >= 1.0f + 0x1p-10f && off <= 0x1p20f;
}

// ---------------------------------------------------------------------------------------
// link residual tables (include/rtuf.h, LINK RESIDUAL TABLES): the class of one drawn pixel and its quantised residual
// ---------------------------------------------------------------------------------------

// One bit per counter of rtuf_link_residuals, in the struct's field order (bit f feeds field f).
enum : uint32_t { kResPixel = 1u, kResInvalid = 2u, kResFiltered = 4u, kResInFront = 8u, kResBehind = 16u, kResAgree = 32u };

// A drawn pixel: sensor value s, the winner's virtual depth v = to_linear_depth(z) and its threshold t.  lo = v - t is the
// filter's compare threshold (shade_threshold: the same float subtraction), so kResFiltered is the mask bit -- for an invalid
// s as well.  q = (s - v) in units of 2^-20 m, round half to even, saturating, NaN -> 0; it counts where kResAgree is set.
RTUF_NUMERIC uint32_t link_residual_class(float s, float v, float t, int& q)
{
  const float lo = __fsub_rn(v, t), hi = __fadd_rn(v, t);
  const bool valid = s > 0.0f, filtered = s > lo, beyond = s > hi;
  q = __float2int_rn(__fmul_rn(__fsub_rn(s, v), 1048576.0f));
  return kResPixel | (valid ? 0u : kResInvalid) | (filtered ? kResFiltered : 0u) | (valid && !filtered ? kResInFront : 0u) |
         (valid && filtered && beyond ? kResBehind : 0u) | (valid && filtered && !beyond ? kResAgree : 0u);
}
// A pixel no fragment reached: it counts as a pixel, and as invalid where the sensor holds no reading.
RTUF_NUMERIC uint32_t link_residual_undrawn(float s) { return kResPixel | (s > 0.0f ? 0u : kResInvalid); }

// ---------------------------------------------------------------------------------------
// filtered point clouds (include/rtuf.h, FILTERED POINT CLOUDS): which sensor values make a point, and the point
// ---------------------------------------------------------------------------------------

// Per-stream intrinsics as the cloud kernels read them: kx = (float)(1.0 / fx), ky = (float)(1.0 / fy), cx, cy.
struct CloudIntrinsics { float kx, ky, cx, cy; };

// A sensor value carries a point iff it is a positive finite number (NaN, 0, -0, negatives and +inf do not).
RTUF_NUMERIC_HD bool cloud_sensor_valid(float s) { return s > 0.0f && s < INFINITY; }

// The point of pixel (u, v) with sensor value s: x = ((u - cx) * s) * kx, y = ((v - cy) * s) * ky, z = s, every operation a
// single float operation in that order (depth_image_proc's association).  Plain operators on host and device alike: a
// difference and two products, nothing an -ffp-contract setting could fuse.
RTUF_NUMERIC_HD void cloud_point(int u, int v, float s, const CloudIntrinsics& k, float& x, float& y, float& z)
{
  const float du = (float)u - k.cx, dv = (float)v - k.cy;
  const float xs = du * s, ys = dv * s;
  x = xs * k.kx;
  y = ys * k.ky;
  z = s;
}

// ---------------------------------------------------------------------------------------
// point list batches (include/rtuf.h, POINT LIST BATCHES): the pixel a point lands on -- the inverse of cloud_point -- and its
// verdict.  Products feed sums here: the includers compile with -ffp-contract=off (the library, tests/point_pixel_check.cpp).
// ---------------------------------------------------------------------------------------

// Per-stream pinhole as the points kernel reads it: fx = (float)fx, fy = (float)fy, cx, cy (beside CloudIntrinsics' kx, ky).
struct PointIntrinsics { float fx, fy, cx, cy; };

// Verdicts of a point.
enum : uint32_t { kPointKept = 0u, kPointFiltered = 1u, kPointOutside = 2u };
constexpr uint32_t kPointNoPixel = 0xffffffffu;

// The optional per-stream transform: m holds the 12 used entries of a column-major matrix as floats, m[4 * c + r] = entry
// (r, c), r < 3 (the last row is not read).  p'_r = ((m[r] x + m[4 + r] y) + m[8 + r] z) + m[12 + r].
RTUF_NUMERIC_HD void point_transform(const float* m, float& x, float& y, float& z)
{
  float o[3];
  for (int r = 0; r < 3; r++) {
    const float a = m[r] * x, b = m[4 + r] * y, c = m[8 + r] * z;
    o[r] = ((a + b) + c) + m[12 + r];
  }
  x = o[0]; y = o[1]; z = o[2];
}

// Is the point judged, and on which pixel does it land?  uf = ((x / z) * fx + cx) + 0.5f, vf likewise (IEEE division); the
// range tests come before the conversions, so no out-of-range float (NaN included) is ever converted and no index outside
// the plane is ever formed.
RTUF_NUMERIC_HD bool point_pixel(float x, float y, float z, const PointIntrinsics& k, int W, int H, int& u, int& v)
{
  u = 0; v = 0;
  if (!(z > 0.0f && z < INFINITY)) return false;
#ifdef __HIP_DEVICE_COMPILE__
  const float a = __fdiv_rn(x, z), b = __fdiv_rn(y, z);
#else
  const float a = x / z, b = y / z;
#endif
  const float au = a * k.fx, bv = b * k.fy;
  const float uf = (au + k.cx) + 0.5f, vf = (bv + k.cy) + 0.5f;
  if (!(uf >= 0.0f && uf < (float)W && vf >= 0.0f && vf < (float)H)) return false;
  u = (int)uf; v = (int)vf;
  return true;
}

// A judged point of depth z against the smallest virtual depth vmin of its window and the threshold t: filtered iff
// z > vmin - t (one float subtraction; vmin = +inf where no link drew, and then nothing is above it).
RTUF_NUMERIC_HD uint32_t point_verdict(float z, float vmin, float t) { return z > vmin - t ? kPointFiltered : kPointKept; }

// ---------------------------------------------------------------------------------------
// voxel occupancy grids (include/rtuf.h, VOXEL OCCUPANCY GRIDS): the voxel a world point falls into.  The point comes from
// cloud_point (plane form) or a list, optionally through point_transform -- the chain above, shared with the point list
// batches.  (tests/voxel_check.cpp against a numpy form, index for index.)
// ---------------------------------------------------------------------------------------

// The grid as the kernels read it: origin and inv = 1.0f / (float)voxel_size as floats, and the dims (each 1 .. 2048, their
// product at most 1 << 27: every index fits 27 bits).
struct VoxelGrid { float ox, oy, oz, inv; int nx, ny, nz; };
constexpr int kMaxVoxelDim = 2048;
constexpr uint32_t kMaxVoxels = 1u << 27;
constexpr uint32_t kVoxelNone = 0xffffffffu;

// g_r = (p_r - o_r) * inv; IN iff 0 <= g_r < (float)dims_r for every r (NaN and infinities fail: nothing is special-cased);
// then i_r = (int)g_r and index = (iz * ny + iy) * nx + ix.  The range tests come before the conversions, as in point_pixel:
// no out-of-range float is ever converted.  index = kVoxelNone for a point that is not IN.
RTUF_NUMERIC_HD bool voxel_of(float x, float y, float z, const VoxelGrid& g, uint32_t& index)
{
  index = kVoxelNone;
  const float dx = x - g.ox, dy = y - g.oy, dz = z - g.oz;
  const float gx = dx * g.inv, gy = dy * g.inv, gz = dz * g.inv;
  if (!(gx >= 0.0f && gx < (float)g.nx && gy >= 0.0f && gy < (float)g.ny && gz >= 0.0f && gz < (float)g.nz)) return false;
  const int ix = (int)gx, iy = (int)gy, iz = (int)gz;
  index = (uint32_t)((iz * g.ny + iy) * g.nx + ix);
  return true;
}

// ---------------------------------------------------------------------------------------
// voxel free space (include/rtuf.h, VOXEL FREE SPACE): the centre of a voxel, the optical_from_world inverse of a stream's
// world_from_optical floats, and the free test.  The centre goes through point_transform and point_pixel above, as they
// stand.  (tests/voxel_free_check.cpp against a numpy form, bit for bit.)
// ---------------------------------------------------------------------------------------

// c_r = o_r + ((float)i_r + 0.5f) * size with size = (float)voxel_size: one add (exact: i_r < 2048), one product, one add.
RTUF_NUMERIC_HD float voxel_centre(int i, float o, float size)
{
  const float h = (float)i + 0.5f;
  const float d = h * size;
  return o + d;
}

// FREE iff z < Emin - m: one float subtraction, strict and ordered (a NaN on either side is not free).
RTUF_NUMERIC_HD bool voxel_free_test(float z, float emin, float m) { return z < emin - m; }

// optical_from_world of the 12 floats m (m[4 * c + r] = entry (r, c), r < 3) the insert uses, in point_transform's layout:
// in double, a(r, c) the floats as doubles, every cofactor one p * q - r * s, det = (a00 C00 + a01 C01) + a02 C02,
// R = adj / det with one division per entry, t'_r = -((R_r0 t_0 + R_r1 t_1) + R_r2 t_2), and only then each of the 12
// results rounded to float.  false -- and out untouched -- when det is 0 or not finite or a result is not finite as a float.
// Host only (once per rtuf_set_voxel_transforms): the includers compile with -ffp-contract=off.
inline bool voxel_inverse_transform(const float* m, float* out)
{
  double a[3][3], t[3];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) a[r][c] = (double)m[4 * c + r];
    t[r] = (double)m[12 + r];
  }
  double C[3][3];      // C[i][j]: the cofactor of a(i, j)
  C[0][0] = a[1][1] * a[2][2] - a[1][2] * a[2][1];
  C[0][1] = a[1][2] * a[2][0] - a[1][0] * a[2][2];
  C[0][2] = a[1][0] * a[2][1] - a[1][1] * a[2][0];
  C[1][0] = a[0][2] * a[2][1] - a[0][1] * a[2][2];
  C[1][1] = a[0][0] * a[2][2] - a[0][2] * a[2][0];
  C[1][2] = a[0][1] * a[2][0] - a[0][0] * a[2][1];
  C[2][0] = a[0][1] * a[1][2] - a[0][2] * a[1][1];
  C[2][1] = a[0][2] * a[1][0] - a[0][0] * a[1][2];
  C[2][2] = a[0][0] * a[1][1] - a[0][1] * a[1][0];
  const double p0 = a[0][0] * C[0][0], p1 = a[0][1] * C[0][1], p2 = a[0][2] * C[0][2];
  const double det = (p0 + p1) + p2;
  if (!(std::isfinite(det) && det != 0.0)) return false;
  float res[16];
  for (int i = 0; i < 16; i++) res[i] = 0.0f;
  for (int r = 0; r < 3; r++) {
    double R[3];
    for (int c = 0; c < 3; c++) R[c] = C[c][r] / det;      // (the adjugate is the cofactors' transpose)
    const double q0 = R[0] * t[0], q1 = R[1] * t[1], q2 = R[2] * t[2];
    const double tr = -((q0 + q1) + q2);
    for (int c = 0; c < 3; c++) res[4 * c + r] = (float)R[c];
    res[12 + r] = (float)tr;
    for (int c = 0; c < 4; c++) if (!std::isfinite(res[4 * c + r])) return false;
  }
  for (int i = 0; i < 16; i++) out[i] = res[i];
  return true;
}

// ---------------------------------------------------------------------------------------
// link clearance tables (include/rtuf.h, LINK CLEARANCE TABLES): a sphere's centre in the camera frame, and the clearance of
// a cloud point to a sphere.  Products feed sums here: both functions need -ffp-contract=off, which the library and the CPU
// check compile with, so that every product and every sum is rounded on its own.
// ---------------------------------------------------------------------------------------

// One row-times-point product chain of a column-major OpenGL matrix: ((m0 x + m4 y) + m8 z) + m12, rows 0 .. 2.
RTUF_NUMERIC_HD void clearance_transform(const double* m, const double p[3], double out[3])
{
  for (int r = 0; r < 3; r++) {
    const double a = m[r] * p[0], b = m[4 + r] * p[1], c = m[8 + r] * p[2];
    out[r] = ((a + b) + c) + m[12 + r];
  }
}

// Centre of a link sphere in the camera's optical frame: offset_inv * (cam_tf * (link_tf * (c, 1))), three matrix-vector
// products in double (the matrices' last rows are not read: they are 0 0 0 1), the result rounded to float.
RTUF_NUMERIC_HD void clearance_centre(const double* link_tf, const double* cam_tf, const double* offset_inv, const float c[3], float out[3])
{
  const double p0[3] = {(double)c[0], (double)c[1], (double)c[2]};
  double p1[3], p2[3], p3[3];
  clearance_transform(link_tf, p0, p1);
  clearance_transform(cam_tf, p1, p2);
  clearance_transform(offset_inv, p2, p3);
  out[0] = (float)p3[0]; out[1] = (float)p3[1]; out[2] = (float)p3[2];
}

// Clearance of point (px, py, pz) to the sphere (cx, cy, cz, r): sqrt((dx dx + dy dy) + dz dz) - r with d = point - centre,
// every operation a single float operation, the square root correctly rounded (sqrtf: IEEE on host and device).
RTUF_NUMERIC_HD float clearance_point_sphere(float px, float py, float pz, float cx, float cy, float cz, float r)
{
  const float dx = px - cx, dy = py - cy, dz = pz - cz;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float d2 = (xx + yy) + zz;
  return sqrtf(d2) - r;
}

// The bits of a clearance (never NaN where it is used, never -0) as an unsigned number of the same order.
RTUF_NUMERIC_HD uint32_t clearance_order_bits(float c)
{
#ifdef __HIP_DEVICE_COMPILE__
  const uint32_t b = __float_as_uint(c);
#else
  uint32_t b; memcpy(&b, &c, 4);
#endif
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
RTUF_NUMERIC_HD uint32_t clearance_bits_of_order(uint32_t o) { return (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o; }

// ---------------------------------------------------------------------------------------
// link padding (include/rtuf.h, LINK PADDING): how far a drawn pixel of a padded link spreads its depth
// ---------------------------------------------------------------------------------------

// The squared reach, in pixels, of a source pixel with window z `z` whose link has `pad` metres of padding, seen through a
// focal length of f pixels: d = num / (z - off) is the shader's to_linear_depth (IEEE division, as shade_threshold's),
// rho = min((pad * f) / d, 16) the projected radius of a ball of `pad` metres at that depth, and the result rho * rho
// truncated -- every operation a single float operation on its own.  The clamp at kMaxLinkPaddingPx = 16 pixels is part of
// the definition: a 2 cm margin reaches it at d = f / 800.  0 where nothing was drawn (NaN) or the pad is 0 (the background's
// slot included).  (tests/link_padding_check.cpp against a numpy form, bit for bit.)
constexpr int kMaxLinkPaddingPx = 16;
RTUF_NUMERIC uint32_t link_padding_reach2(float z, float pad, float f, float num, float off)
{
  if (!(z == z) || !(pad > 0.0f)) return 0u;
  const float d = __fdiv_rn(num, __fsub_rn(z, off));
  const float rho = fminf(__fdiv_rn(__fmul_rn(pad, f), d), (float)kMaxLinkPaddingPx);
  return (uint32_t)__fmul_rn(rho, rho);
}

// ---------------------------------------------------------------------------------------
// scene planes (include/rtuf.h, SCENE PLANES): what lies at or behind a stream's learned depth plane is filtered too
// ---------------------------------------------------------------------------------------

// thr = scene - (abs_m + rel * scene), every operation a single float operation rounded on its own.  An unknown scene pixel
// (+inf or NaN) gives NaN for every legal margin (abs_m >= 0 finite, 0 <= rel < 1): rel * inf is inf, or NaN for rel = 0, and
// inf - (abs_m + inf) = inf - inf = NaN -- no sensor value is above a NaN, so nothing is special-cased.
// (tests/scene_check.cpp against a numpy form, bit for bit.)
RTUF_NUMERIC float scene_threshold(float scene, float abs_m, float rel)
{
  return __fsub_rn(scene, __fadd_rn(abs_m, __fmul_rn(rel, scene)));
}
// Strict and ordered: a NaN sensor value is never scene-filtered.
RTUF_NUMERIC bool scene_filtered(float s, float scene, float abs_m, float rel) { return s > scene_threshold(scene, abs_m, rel); }

// Learning (rtuf_learn_scene_batch*): a pixel the ROBOT filter keeps and whose reading carries a point lowers the plane to that
// reading -- a running minimum of input values, so idempotent and independent of the frames' order.  A NaN plane value is
// "unknown" like +inf: the first such reading replaces it (fminf's rule).
RTUF_NUMERIC float scene_learned(float scene, float s, bool robot_filtered)
{
  return !robot_filtered && cloud_sensor_valid(s) && !(scene <= s) ? s : scene;
}

// ---------------------------------------------------------------------------------------
// set-up kernel: the list counters of a work item (tests/setup_lists_check.cpp)
// ---------------------------------------------------------------------------------------

// The three survivor lists of an item (records, <= 2x2 boxes, <= 4x4 boxes) hold at most 3 x 256 = 768 entries TOGETHER, so
// their three counters are 10-bit fields of one word and one addition reserves in all three; no field can carry into the next.
constexpr uint32_t kListFieldBits = 10u, kListFieldMask = (1u << kListFieldBits) - 1u;
RTUF_NUMERIC_HD uint32_t list_counts(uint32_t nrec, uint32_t ntiny, uint32_t nsmall)
{
  return nrec | (ntiny << kListFieldBits) | (nsmall << (2u * kListFieldBits));
}
RTUF_NUMERIC_HD uint32_t list_count_rec(uint32_t w) { return w & kListFieldMask; }
RTUF_NUMERIC_HD uint32_t list_count_tiny(uint32_t w) { return (w >> kListFieldBits) & kListFieldMask; }
RTUF_NUMERIC_HD uint32_t list_count_small(uint32_t w) { return (w >> (2u * kListFieldBits)) & kListFieldMask; }

#ifdef __HIP__
// The IEEE division without the instructions that only matter for operands near the ends of the exponent range: the compiler
// expands a correctly rounded a / b into v_div_scale_f32 twice (operand pre-scaling), v_rcp_f32, one Newton step, the quotient
// with two residual corrections (the last as v_div_fmas_f32, which undoes the scaling) and v_div_fixup_f32 (zero / infinite /
// NaN / denormal operands).  With both operands and the quotient far inside the normal range the scalings are identities and
// the fix-up returns its input, and what is left is this: one v_rcp_f32 and seven 2-cycle instructions instead of eleven, four
// of them in the 4-cycle class.  scripts/fdiv_check.hip compares it with __fdiv_rn for every float z in [-1, 1 + 2^-11] on the
// GPU: 0 of 5.75e10 quotients differ inside the domain fast_div_admitted admits, and the two pairs outside it (z_far 10,000 x
// z_near) show what the rule is for -- there z - off passes through zero and the fix-up's infinity is not what the core
// returns (profiles/r06_experiment_fast_class_batches_2_3.txt).
__device__ __forceinline__ float div_core(float n, float d)
{
  float r = __builtin_amdgcn_rcpf(d);
  const float e = __fmaf_rn(-d, r, 1.0f);
  r = __fmaf_rn(e, r, r);
  float q = __fmul_rn(n, r);
  float res = __fmaf_rn(-d, q, n);
  q = __fmaf_rn(res, r, q);
  res = __fmaf_rn(-d, q, n);
  return __fmaf_rn(res, r, q);
}
#endif

}  // namespace rtuf
