// Depthwise 3x3 convolution with optional ReLU6 on the source and on the output: the middle layer of the reference's inverted-residual block
// (models/CNNs.py InvertedResidual :159-185: conv1x1 C -> 4C + ReLU6, depthwise conv3x3 + ReLU6, conv1x1 4C -> C, + x).  The two 1x1 convolutions
// run on the existing kernels without an activation; both ReLU6 are applied here, the first to the source element as it is staged.
//   forward   a = act_out( sum_{ky,kx} w[c,ky,kx] * act_src(e)[y+ky-1, x+kx-1, c] + b[c] )                     out-of-image taps contribute 0
//   data      g = da * act_out'(a);   de = act_src'(e) * sum_{ky,kx} w[c,ky,kx] * g[y-ky+1, x-kx+1, c]          one launch, g formed on load
//   weight    dW[c,ky,kx] = sum_{n,y,x} g * act_src(e)[y+ky-1, x+kx-1, c];   db[c] = sum g                      two ordered stages, no atomics
// ReLU6' is torch's: 1 only where 0 < v < 6, strictly; act_out' is taken from the stored (rounded) output a, so no pre-activation tensor exists.
// Channels-last (N, H, W, C), fp32 or bf16, stride 1, zero padding 1; the (C, 1, 3, 3) fp32 weight and the (C) fp32 bias are read as stored.
// Arithmetic in fp32 registers, one rounding at the store.
//
// One workgroup of 256 threads owns a DW_TH x DW_TW pixel tile of one image and a block of CV * VN channels.  It stages the tile with its
// one-pixel halo in LDS ONCE, already activated (forward, weight gradient: act_src(e)) or already masked (data gradient: g), in the
// tensor's own type -- ReLU6 of a bf16 and a bf16 times 0 or 1 are bf16 values, nothing is rounded by the staging -- so every element is
// fetched from memory and clamped once per tile; the nine taps are LDS reads.  A thread owns one channel vector (its nine weights per channel
// stay in registers) and every (256 / CV)-th pixel of the tile.
// Two routes (vmg_dwconv3_plan): VECTOR, VN = 16 bytes (8 bf16 / 4 fp32), CV = 8, where C is a multiple of VN and every activation pointer
// is 16-byte aligned; ELEMENT, VN = 1, CV = 32, for any C and any element-aligned pointer.
// Addressing: the plan REFUSES N * H * W * C >= 2^31 (a clear error, no launch).  Element offsets are nevertheless formed in 64 bits.
#include "common.h"

namespace {

constexpr int DW_TH = 8, DW_TW = 16;                // pixel tile
constexpr int DW_HW = DW_TW + 2;                    // halo tile width
constexpr int DW_HALO = (DW_TH + 2) * (DW_TW + 2);  // pixels staged per tile
constexpr int DW_MAX_PARTIALS = 128;                // first-stage workgroups per channel block of the weight gradient, at most

template <typename T, int VN>
struct alignas(sizeof(T) * VN) DwVec { T v[VN]; };

__device__ __forceinline__ float relu6_f(float v) { return v < 0.f ? 0.f : (v > 6.f ? 6.f : v); }
__device__ __forceinline__ bool relu6_open(float v) { return v > 0.f && v < 6.f; }

// tile[(hy * DW_HW + hx) * CV + cv] <- the staged value of image pixel (y0 - 1 + hy, x0 - 1 + hx), channels (cv0 + cv) * VN .. + VN - 1 of image
// `img` (an element offset); zero outside the image and beyond C.
//   MASKED false: act ? relu6(p) : p                        (act_src(e))
//   MASKED true:  act ? (0 < q < 6 ? p : 0) : p             (g = da * act_out'(a), p = da, q = a)
template <typename T, int VN, int CV, bool MASKED>
__device__ __forceinline__ void dw_stage(DwVec<T, VN>* tile, const T* __restrict__ p, const T* __restrict__ q, int act, long long img, int y0, int x0,
                                         int H, int W, int C, int cv0) {
  typedef DwVec<T, VN> Vec;
  // The element route issues a thread's whole share of loads (23 single elements) before it uses the first: measured 170 -> 141 us forward at
  // 28 x 64 x 64 x 575 bf16.  The vector route keeps one 16-byte load in flight per thread: with six vectors (and six mask vectors) held
  // next to the nine weights per channel it lost a wave per SIMD and ran slower (96 -> 110 us at 576 channels).
  constexpr int IT = VN == 1 ? (DW_HALO * CV + 255) / 256 : 1;
  for (int i0 = threadIdx.x; i0 < DW_HALO * CV; i0 += 256 * IT) {
    Vec r[IT], m[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = i0 + it * 256;
      const int hp = i / CV, cv = i - hp * CV;
      const int hy = hp / DW_HW, hx = hp - hy * DW_HW;
      const int y = y0 - 1 + hy, x = x0 - 1 + hx, c = (cv0 + cv) * VN;
      // (an i beyond the tile has hy >= DW_TH + 2: read if that pixel happens to be in the image, never stored.  VN > 1 only where C % VN == 0:
      // a vector is wholly inside or wholly outside)
      if (y >= 0 && y < H && x >= 0 && x < W && c < C) {
        const long long off = img + ((long long)y * W + x) * C + c;
        r[it] = *reinterpret_cast<const Vec*>(p + off);
        if (MASKED && act) m[it] = *reinterpret_cast<const Vec*>(q + off);
      } else {
#pragma unroll
        for (int e = 0; e < VN; ++e) {
          r[it].v[e] = from_f32<T>(0.f);
          if (MASKED) m[it].v[e] = from_f32<T>(0.f);
        }
      }
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = i0 + it * 256;
      if (act) {
#pragma unroll
        for (int e = 0; e < VN; ++e) {
          if (MASKED) {
            if (!relu6_open(to_f32(m[it].v[e]))) r[it].v[e] = from_f32<T>(0.f);
          } else {
            r[it].v[e] = from_f32<T>(relu6_f(to_f32(r[it].v[e])));
          }
        }
      }
      if (i < DW_HALO * CV) tile[i] = r[it];
    }
  }
}

// blockIdx.x = ((n * tY + ty) * tX + tx) * cbs + cb
// BWD false: in = e, out = a.   BWD true: in = da, aux = a (read if out_act), xref = e (read if src_act), out = de; bias unused.
template <typename T, int VN, int CV, bool BWD>
__global__ __launch_bounds__(256) void dwconv3_kernel(const T* __restrict__ in, const T* __restrict__ aux, const T* __restrict__ xref,
                                                      const float* __restrict__ w, const float* __restrict__ bias, T* __restrict__ out, int H, int W,
                                                      int C, int tY, int tX, int cbs, int src_act, int out_act) {
  typedef DwVec<T, VN> Vec;
  __shared__ Vec tile[DW_HALO * CV];
  constexpr int PG = 256 / CV;
  unsigned b = blockIdx.x;
  const int cb = (int)(b % (unsigned)cbs);
  b /= (unsigned)cbs;
  const int tx = (int)(b % (unsigned)tX);
  b /= (unsigned)tX;
  const int ty = (int)(b % (unsigned)tY);
  const int n = (int)(b / (unsigned)tY);
  const int y0 = ty * DW_TH, x0 = tx * DW_TW;
  const long long img = (long long)n * H * W * C;
  if (BWD) dw_stage<T, VN, CV, true>(tile, in, aux, out_act, img, y0, x0, H, W, C, cb * CV);
  else dw_stage<T, VN, CV, false>(tile, in, nullptr, src_act, img, y0, x0, H, W, C, cb * CV);
  __syncthreads();
  const int cv = threadIdx.x % CV, pg = threadIdx.x / CV;
  const int c = (cb * CV + cv) * VN;
  if (c >= C) return;
  float wk[9][VN], bk[VN];
#pragma unroll
  for (int e = 0; e < VN; ++e) {
#pragma unroll
    for (int k = 0; k < 9; ++k) wk[k][e] = w[(long long)(c + e) * 9 + k];
    bk[e] = BWD ? 0.f : bias[c + e];
  }
  // (the element route's 16 pixels per thread are unrolled: 170 -> 141 us with the staging above; the vector route's four stay a loop, unrolled they
  // cost registers and a wave per SIMD)
#pragma unroll(VN == 1 ? DW_TH * DW_TW / PG : 1)
  for (int j = 0; j < DW_TH * DW_TW / PG; ++j) {
    const int p = pg + j * PG;
    const int py = p / DW_TW, px = p - py * DW_TW;
    const int y = y0 + py, x = x0 + px;
    if (y >= H || x >= W) continue;
    float acc[VN];
#pragma unroll
    for (int e = 0; e < VN; ++e) acc[e] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        // forward: the source pixel (y + ky - 1, x + kx - 1) is halo pixel (py + ky, px + kx); data gradient: (y - ky + 1, x - kx + 1) is (py + 2 - ky, px + 2 - kx)
        const int hy = BWD ? py + 2 - ky : py + ky, hx = BWD ? px + 2 - kx : px + kx;
        const Vec v = tile[(hy * DW_HW + hx) * CV + cv];
#pragma unroll
        for (int e = 0; e < VN; ++e) acc[e] += wk[ky * 3 + kx][e] * to_f32(v.v[e]);
      }
    const long long off = img + ((long long)y * W + x) * C + c;
    Vec r;
    if (BWD) {
      if (src_act) {
        const Vec s = *reinterpret_cast<const Vec*>(xref + off);
#pragma unroll
        for (int e = 0; e < VN; ++e) r.v[e] = from_f32<T>(relu6_open(to_f32(s.v[e])) ? acc[e] : 0.f);
      } else {
#pragma unroll
        for (int e = 0; e < VN; ++e) r.v[e] = from_f32<T>(acc[e]);
      }
    } else {
#pragma unroll
      for (int e = 0; e < VN; ++e) {
        const float t = acc[e] + bk[e];
        r.v[e] = from_f32<T>(out_act ? relu6_f(t) : t);
      }
    }
    *reinterpret_cast<Vec*>(out + off) = r;
  }
}

// Weight gradient, first stage.  blockIdx.x = part * cbs + cb: the workgroup walks the tiles [tiles * part / P, tiles * (part + 1) / P) of the
// (n, ty, tx) order, stages act_src(e) of each as the forward does, forms g = da * act_out'(a) on load and keeps 9 + 1 running sums per
// channel in registers.  The 256 / CV pixel lanes of a channel are then added through LDS in lane order and the sums written to
// ws[(part * C + c) * 10 + k] (k = ky * 3 + kx; k = 9: the bias).  Which pixels a lane sums, and in which order, depends on the geometry alone.
template <typename T, int VN, int CV>
__global__ __launch_bounds__(256) void dwconv3_wgrad_kernel(const T* __restrict__ src, const T* __restrict__ da, const T* __restrict__ a,
                                                            float* __restrict__ ws, int H, int W, int C, int tY, int tX, int cbs, long long tiles, int P,
                                                            int src_act, int out_act) {
  typedef DwVec<T, VN> Vec;
  __shared__ Vec tile[DW_HALO * CV];
  __shared__ float red[VN * 256];
  constexpr int PG = 256 / CV;
  const int cb = (int)(blockIdx.x % (unsigned)cbs), part = (int)(blockIdx.x / (unsigned)cbs);
  const int cv = threadIdx.x % CV, pg = threadIdx.x / CV;
  const int c = (cb * CV + cv) * VN;
  float acc[10][VN];
#pragma unroll
  for (int k = 0; k < 10; ++k)
#pragma unroll
    for (int e = 0; e < VN; ++e) acc[k][e] = 0.f;
  const long long t0 = tiles * part / P, t1 = tiles * (part + 1) / P;
  for (long long t = t0; t < t1; ++t) {
    const int tx = (int)(t % tX);
    const long long r = t / tX;
    const int ty = (int)(r % tY), n = (int)(r / tY);
    const int y0 = ty * DW_TH, x0 = tx * DW_TW;
    const long long img = (long long)n * H * W * C;
    __syncthreads();  // (the previous tile's readers are done)
    dw_stage<T, VN, CV, false>(tile, src, nullptr, src_act, img, y0, x0, H, W, C, cb * CV);
    __syncthreads();
    if (c < C) {
      for (int i = 0; i < DW_TH * DW_TW / PG; ++i) {
        const int p = pg + i * PG;
        const int py = p / DW_TW, px = p - py * DW_TW;
        const int y = y0 + py, x = x0 + px;
        if (y >= H || x >= W) continue;
        const long long off = img + ((long long)y * W + x) * C + c;
        const Vec d = *reinterpret_cast<const Vec*>(da + off);
        float g[VN];
        if (out_act) {
          const Vec m = *reinterpret_cast<const Vec*>(a + off);
#pragma unroll
          for (int e = 0; e < VN; ++e) g[e] = relu6_open(to_f32(m.v[e])) ? to_f32(d.v[e]) : 0.f;
        } else {
#pragma unroll
          for (int e = 0; e < VN; ++e) g[e] = to_f32(d.v[e]);
        }
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const Vec v = tile[((py + ky) * DW_HW + px + kx) * CV + cv];
#pragma unroll
            for (int e = 0; e < VN; ++e) acc[ky * 3 + kx][e] += g[e] * to_f32(v.v[e]);
          }
#pragma unroll
        for (int e = 0; e < VN; ++e) acc[9][e] += g[e];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < VN; ++e) red[e * 256 + threadIdx.x] = acc[k][e];
    __syncthreads();
    if (threadIdx.x < CV * VN) {
      const int cv2 = threadIdx.x / VN, e = threadIdx.x - cv2 * VN;
      const int c2 = (cb * CV + cv2) * VN + e;
      if (c2 < C) {
        float s = 0.f;
        for (int j = 0; j < PG; ++j) s += red[e * 256 + j * CV + cv2];
        ws[((long long)part * C + c2) * 10 + k] = s;
      }
    }
  }
}

// second stage: one thread per (c, k) adds the P partials in index order; written (accumulate 0) or added to dW / db (1)
__global__ __launch_bounds__(256) void dwconv3_wgrad_final_kernel(const float* __restrict__ ws, float* __restrict__ dW, float* __restrict__ db, int C, int P,
                                                                  int accumulate) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= (long long)C * 10) return;
  const int c = (int)(i / 10), k = (int)(i - (long long)c * 10);
  float s = 0.f;
  for (int p = 0; p < P; ++p) s += ws[((long long)p * C + c) * 10 + k];
  float* dst = k < 9 ? dW + (long long)c * 9 + k : db + c;
  *dst = accumulate ? *dst + s : s;
}

struct DwPlan { int route, cb, grid, lds, partials, wgrid, tY, tX, cbs; };

// N * H * W * C (every factor at least 1), saturated at 2^31: the product is never formed beyond 2^62
long long dw_elems(int N, int H, int W, int C) {
  long long v = N;
  const int f[3] = {H, W, C};
  for (int i = 0; i < 3; ++i) v = v >= (1LL << 31) ? v : v * f[i];
  return v >= (1LL << 31) ? (1LL << 31) : v;
}

// the one place the geometry is decided; false (with the error text set) when the shape is refused
bool dw_plan(const char* who, int dtype, int N, int H, int W, int C, int aligned16, DwPlan* p) {
  if (dtype != VMG_F32 && dtype != VMG_BF16) { vmg_set_error("%s: bad dtype", who); return false; }
  if (N < 1 || H < 1 || W < 1 || C < 1) { vmg_set_error("%s: N, H, W and C must be at least 1", who); return false; }
  const long long elems = dw_elems(N, H, W, C);
  if (elems >= (1LL << 31)) {
    vmg_set_error("%s: N * H * W * C = %d * %d * %d * %d: tensors of 2^31 elements or more are refused", who, N, H, W, C);
    return false;
  }
  const int es = dtype == VMG_BF16 ? 2 : 4, vn = 16 / es;
  const bool vec = aligned16 && C % vn == 0;
  p->route = vec ? VMG_DWCONV_VECTOR : VMG_DWCONV_ELEMENT;
  const int cv = vec ? 8 : 32;
  p->cb = vec ? cv * vn : cv;
  p->tY = cdiv(H, DW_TH);
  p->tX = cdiv(W, DW_TW);
  p->cbs = cdiv(C, p->cb);
  const long long tiles = (long long)N * p->tY * p->tX;
  p->grid = (int)(tiles * p->cbs);  // < 2^31: a workgroup covers at least one element
  p->lds = DW_HALO * cv * (vec ? 16 : es);
  p->partials = (int)(tiles < DW_MAX_PARTIALS ? tiles : DW_MAX_PARTIALS);
  p->wgrid = p->partials * p->cbs;
  return true;
}

}  // namespace

extern "C" int vmg_dwconv3_plan(int dtype, int N, int H, int W, int C, int aligned16, int* plan) {
  VMG_CHECK(plan != nullptr, "dwconv3_plan: null result");
  DwPlan p;
  if (!dw_plan("dwconv3_plan", dtype, N, H, W, C, aligned16, &p)) return -1;
  plan[0] = p.route; plan[1] = DW_TH; plan[2] = DW_TW; plan[3] = p.cb;
  plan[4] = p.grid; plan[5] = p.lds; plan[6] = p.partials; plan[7] = p.wgrid;
  return 0;
}

extern "C" int64_t vmg_dwconv3_wgrad_ws_bytes(int dtype, int N, int H, int W, int C) {
  DwPlan p;
  if (!dw_plan("dwconv3_wgrad_ws_bytes", dtype, N, H, W, C, 0, &p)) return -1;
  return (int64_t)p.partials * C * 10 * (int64_t)sizeof(float);  // (the partial count does not depend on the route)
}

static int dw_common(const char* who, int dtype, int src_act, int out_act, int N, int H, int W, int C, uintptr_t bits, DwPlan* p) {
  VMG_CHECK(dtype == VMG_F32 || dtype == VMG_BF16, "%s: bad dtype", who);
  VMG_CHECK((src_act == 0 || src_act == 1) && (out_act == 0 || out_act == 1), "%s: src_act and out_act are 0 (none) or 1 (ReLU6)", who);
  const int es = dtype == VMG_BF16 ? 2 : 4;
  VMG_CHECK(bits % es == 0, "%s: activation pointers must be aligned to the element size (%d bytes)", who, es);
  return dw_plan(who, dtype, N, H, W, C, bits % 16 == 0, p) ? 0 : -1;
}

// (the launch is a statement with commas of its own: it travels through the macros as their variadic tail)
#define VMG_DW_ROUTE(T_, VN_, CV_, ...) \
  do {                                  \
    constexpr int VN = VN_, CV = CV_;   \
    typedef T_ T;                       \
    __VA_ARGS__;                        \
  } while (0)
#define VMG_DW_DISPATCH(...)                                                    \
  do {                                                                          \
    if (dtype == VMG_BF16) {                                                    \
      if (p.route == VMG_DWCONV_VECTOR) VMG_DW_ROUTE(bf16, 8, 8, __VA_ARGS__);  \
      else VMG_DW_ROUTE(bf16, 1, 32, __VA_ARGS__);                              \
    } else {                                                                    \
      if (p.route == VMG_DWCONV_VECTOR) VMG_DW_ROUTE(float, 4, 8, __VA_ARGS__); \
      else VMG_DW_ROUTE(float, 1, 32, __VA_ARGS__);                             \
    }                                                                           \
  } while (0)

extern "C" int vmg_dwconv3_fwd(int dtype, int src_act, int out_act, const void* e, const float* w, const float* b, void* a, int N, int H, int W, int C,
                               void* stream) {
  VMG_CHECK(e && w && b && a, "dwconv3_fwd: null pointer");
  VMG_CHECK(((uintptr_t)w | (uintptr_t)b) % 4 == 0, "dwconv3_fwd: weight and bias must be 4-byte aligned");
  DwPlan p;
  if (dw_common("dwconv3_fwd", dtype, src_act, out_act, N, H, W, C, (uintptr_t)e | (uintptr_t)a, &p)) return -1;
  hipStream_t st = (hipStream_t)stream;
  VMG_DW_DISPATCH(hipLaunchKernelGGL((dwconv3_kernel<T, VN, CV, false>), dim3(p.grid), dim3(256), 0, st, (const T*)e, (const T*)nullptr, (const T*)nullptr, w, b,
                                      (T*)a, H, W, C, p.tY, p.tX, p.cbs, src_act, out_act));
  VMG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vmg_dwconv3_bwd_data(int dtype, int src_act, int out_act, const void* da, const void* a, const void* e, const float* w, void* de, int N,
                                    int H, int W, int C, void* stream) {
  VMG_CHECK(da && w && de, "dwconv3_bwd_data: null pointer");
  VMG_CHECK((src_act == 0 || src_act == 1) && (out_act == 0 || out_act == 1), "dwconv3_bwd_data: src_act and out_act are 0 (none) or 1 (ReLU6)");
  VMG_CHECK((a || !out_act) && (e || !src_act), "dwconv3_bwd_data: null pointer (a is read with out_act, e with src_act)");
  VMG_CHECK((uintptr_t)w % 4 == 0, "dwconv3_bwd_data: the weight must be 4-byte aligned");
  DwPlan p;
  const uintptr_t bits = (uintptr_t)da | (uintptr_t)de | (out_act ? (uintptr_t)a : 0) | (src_act ? (uintptr_t)e : 0);
  if (dw_common("dwconv3_bwd_data", dtype, src_act, out_act, N, H, W, C, bits, &p)) return -1;
  hipStream_t st = (hipStream_t)stream;
  VMG_DW_DISPATCH(hipLaunchKernelGGL((dwconv3_kernel<T, VN, CV, true>), dim3(p.grid), dim3(256), 0, st, (const T*)da, (const T*)a, (const T*)e, w,
                                      (const float*)nullptr, (T*)de, H, W, C, p.tY, p.tX, p.cbs, src_act, out_act));
  VMG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vmg_dwconv3_bwd_weight(int dtype, int src_act, int out_act, const void* da, const void* a, const void* e, float* dW, float* db, int N, int H,
                                      int W, int C, int accumulate, void* ws, int64_t ws_bytes, void* stream) {
  VMG_CHECK(da && e && dW && db && ws, "dwconv3_bwd_weight: null pointer");
  VMG_CHECK((src_act == 0 || src_act == 1) && (out_act == 0 || out_act == 1), "dwconv3_bwd_weight: src_act and out_act are 0 (none) or 1 (ReLU6)");
  VMG_CHECK(a || !out_act, "dwconv3_bwd_weight: null pointer (a is read with out_act)");
  VMG_CHECK(accumulate == 0 || accumulate == 1, "dwconv3_bwd_weight: accumulate is 0 or 1");
  VMG_CHECK(((uintptr_t)dW | (uintptr_t)db | (uintptr_t)ws) % 4 == 0, "dwconv3_bwd_weight: dW, db and ws must be 4-byte aligned");
  DwPlan p;
  const uintptr_t bits = (uintptr_t)da | (uintptr_t)e | (out_act ? (uintptr_t)a : 0);
  if (dw_common("dwconv3_bwd_weight", dtype, src_act, out_act, N, H, W, C, bits, &p)) return -1;
  VMG_CHECK((int64_t)p.partials * C * 10 * (int64_t)sizeof(float) <= ws_bytes, "dwconv3_bwd_weight: workspace too small (vmg_dwconv3_wgrad_ws_bytes)");
  hipStream_t st = (hipStream_t)stream;
  const long long tiles = (long long)N * p.tY * p.tX;
  VMG_DW_DISPATCH(hipLaunchKernelGGL((dwconv3_wgrad_kernel<T, VN, CV>), dim3(p.wgrid), dim3(256), 0, st, (const T*)e, (const T*)da, (const T*)a, (float*)ws, H, W,
                                      C, p.tY, p.tX, p.cbs, tiles, p.partials, src_act, out_act));
  VMG_LAUNCH_CHECK();
  hipLaunchKernelGGL(dwconv3_wgrad_final_kernel, dim3((unsigned)cdiv64((int64_t)C * 10, 256)), dim3(256), 0, st, (const float*)ws, dW, db, C, p.partials, accumulate);
  VMG_LAUNCH_CHECK();
  return 0;
}
#undef VMG_DW_DISPATCH
#undef VMG_DW_ROUTE
