// Kernels of the patch-shift FFN, Mlp_cnn_shift (reference: models/function.py PatchShift2D :197-236 and the FFN built on it):
//   x1 = gelu(fc(x));  h = shift_inv(gelu(fc1(shift(x1))));  w = gelu(fc2(x1));  a = softmax_2(reweight(mean(h + w)));  y = proj(h a0 + w a1)
// The Linears and the pooled mean run on the existing kernels (conv_igemm.hip KS = 1, vmg_group_reduce mode 0).  Here: the per-channel-chunk
// spatial shift (forward and backward, optionally with an exact GELU on the source element), the two-branch softmax SE MLP, the two-branch
// gradient reduction and the two-branch mix.  Everything is channels-last, fp32 or bf16, arithmetic in fp32 registers; no LDS beyond the
// reductions' ordered partials, no atomics, no allocation, no synchronisation.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ patch shift
// PatchShift2D in closed form, for (N, H, W, Cs): g = ceil(Cs / 9), channel c belongs to chunk i = c / g (trailing chunks may be partly or
// wholly absent), and   out[n, y, x, c] = f(in[n, y - s (1 - i/3), x - s (1 - i%3), c]),   zero where the source pixel is outside the frame
// (the reference's one-pixel zero pad absorbs the roll: nothing wraps, nothing moves between frames).  s = +1 shift, s = -1 shift_inv.
// One thread per VN channels of one DESTINATION pixel, consecutive lanes along the channels: the lanes of a chunk read one contiguous run.
// VN = 16 bytes when chunk boundaries fall on vector boundaries (g % VN == 0), else 1: the per-element form is right for any g.
//   PS_COPY      dst = shifted src                          (also the backward of the identity form: the adjoint of sign s is sign -s)
//   PS_GELU_FWD  dst = shifted gelu(src)                    (gelu(0) = 0: the zero fill is the same)
//   PS_GELU_BWD  dst = gelu'(xref) * shifted src            (src = dy, gathered with the opposite sign by the host entry; xref at the destination)
// Every load is unconditional: a lane whose source is outside the frame reads its own destination offset (in bounds) and discards it.
enum { PS_COPY = 0, PS_GELU_FWD = 1, PS_GELU_BWD = 2 };

template <typename T, int VN, int MODE>
__global__ __launch_bounds__(256) void patch_shift_kernel(const T* __restrict__ src, const T* __restrict__ xref, T* __restrict__ dst, long long total,
                                                          int H, int W, int Cs, int g, int sign) {
  struct alignas(sizeof(T) * VN) Vec { T v[VN]; };
  const int nvec = Cs / VN;
  const bool small = total < (1LL << 31);  // (uniform: the usual case divides in 32 bits)
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    int v, x, y;
    if (small) {
      const unsigned pix = (unsigned)i / (unsigned)nvec;
      v = (int)((unsigned)i - pix * (unsigned)nvec);
      const unsigned row = pix / (unsigned)W;
      x = (int)(pix - row * (unsigned)W);
      y = (int)(row % (unsigned)H);
    } else {
      const long long pix = i / nvec;
      v = (int)(i - pix * nvec);
      const long long row = pix / W;
      x = (int)(pix - row * W);
      y = (int)(row % H);
    }
    const int chunk = (v * VN) / g;  // 0 .. 8
    const int oy = sign * (1 - chunk / 3), ox = sign * (1 - chunk % 3);
    const int sy = y - oy, sx = x - ox;
    const bool ok = sy >= 0 && sy < H && sx >= 0 && sx < W;
    const long long off = i * VN;  // = pixel * Cs + v * VN
    const long long soff = ok ? off - ((long long)oy * W + ox) * Cs : off;
    const Vec a = *reinterpret_cast<const Vec*>(src + soff);
    Vec r;
    if (MODE == PS_GELU_BWD) {
      const Vec q = *reinterpret_cast<const Vec*>(xref + off);
#pragma unroll
      for (int e = 0; e < VN; ++e) r.v[e] = from_f32<T>(ok ? gelu_erf_grad(to_f32(q.v[e])) * to_f32(a.v[e]) : 0.f);
    } else if (MODE == PS_GELU_FWD) {
#pragma unroll
      for (int e = 0; e < VN; ++e) r.v[e] = from_f32<T>(ok ? gelu_erf(to_f32(a.v[e])) : 0.f);
    } else {
#pragma unroll
      for (int e = 0; e < VN; ++e) r.v[e] = ok ? a.v[e] : from_f32<T>(0.f);
    }
    *reinterpret_cast<Vec*>(dst + off) = r;
  }
}

// ------------------------------------------------------------------------------------------------ two-branch reduction
// partial[g][chunk][c][k] = sum over the chunk's rows of a * b_k (k = 0, 1): the two branch sums of the re-weighting backward (d softmax
// weights) from ONE pass over a = dy.  The blocking of vmg_group_reduce3 (tab_ops.hip): threads along VN-channel vectors, 256 / (C / VN)
// rows per block iteration, the row partials combined through LDS in a fixed order, block partials to the workspace; reduce2_final_kernel
// adds a group's chunks in index order.  No atomics: the same bits on every run.
template <typename T, int VN>
__global__ __launch_bounds__(256) void reduce2_kernel(const T* __restrict__ a, const T* __restrict__ b0, const T* __restrict__ b1,
                                                      float* __restrict__ out, long long R, int C, int chunks) {
  struct alignas(sizeof(T) * VN) Vec { T v[VN]; };
  __shared__ float red[2 * VN * 256];
  const int g = blockIdx.x / chunks, ck = blockIdx.x - g * chunks;
  const int tpr = C / VN;
  const int rpb = 256 / tpr;
  const int roff = threadIdx.x / tpr, cp = threadIdx.x - roff * tpr;
  const long long r0 = R * ck / chunks, r1 = R * (ck + 1) / chunks;
  float s[2][VN];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int e = 0; e < VN; ++e) s[k][e] = 0.f;
  if (roff < rpb) {
    const long long base = (long long)g * R * C + VN * cp;
    for (long long r = r0 + roff; r < r1; r += rpb) {
      const long long o = base + r * C;
      const Vec va = *reinterpret_cast<const Vec*>(a + o);
      const Vec v0 = *reinterpret_cast<const Vec*>(b0 + o), v1 = *reinterpret_cast<const Vec*>(b1 + o);
#pragma unroll
      for (int e = 0; e < VN; ++e) {
        const float d = to_f32(va.v[e]);
        s[0][e] += d * to_f32(v0.v[e]);
        s[1][e] += d * to_f32(v1.v[e]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int e = 0; e < VN; ++e) red[(k * VN + e) * 256 + threadIdx.x] = s[k][e];
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += 256) {
    const int c = i >> 1, k = i & 1;
    const int cp2 = c / VN, e = c - cp2 * VN;
    float t = 0.f;
    for (int j = 0; j < rpb; ++j) t += red[(k * VN + e) * 256 + j * tpr + cp2];
    out[(((long long)g * chunks + ck) * C + c) * 2 + k] = t;
  }
}

// out[g, i] = scale * sum over the group's chunks of partial[g][chunk][i], i < width = 2 C.  One block per (group, 16 columns): row group q
// adds the chunks q, q + 16, ... in that order, the 16 row-group sums are then added in index order through LDS -- a fixed summation tree.
__global__ __launch_bounds__(256) void reduce2_final_kernel(const float* __restrict__ partial, float* __restrict__ out, int chunks, int width, float scale) {
  __shared__ float sm[16][17];
  const int slabs = (width + 15) >> 4;
  const int g = blockIdx.x / slabs, c = (blockIdx.x - g * slabs) * 16 + (threadIdx.x & 15);
  const int q = threadIdx.x >> 4;
  float t = 0.f;
  if (c < width) {
    const float* p = partial + (long long)g * chunks * width + c;
    for (int k = q; k < chunks; k += 16) t += p[(long long)k * width];
  }
  sm[q][threadIdx.x & 15] = t;
  __syncthreads();
  if (q == 0 && c < width) {
    float u = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) u += sm[i][threadIdx.x & 15];
    out[(long long)g * width + c] = u * scale;
  }
}

// ------------------------------------------------------------------------------------------------ two-branch mix
// forward   y = h * a[g, c, 0] + w * a[g, c, 1]                              (p0 = h, p1 = w, o0 = y)
// backward  dh = dy * a[g, c, 0] + dm[g, c];  dw = dy * a[g, c, 1] + dm[g, c]  (p0 = dy, o0 = dh, o1 = dw: one launch, two outputs)
// a (G, C, 2) and dm (G, C) fp32; R rows per group.
template <typename T, int VN, bool BWD>
__global__ __launch_bounds__(256) void mix2_kernel(const T* __restrict__ p0, const T* __restrict__ p1, const float* __restrict__ coef,
                                                   const float* __restrict__ add, T* __restrict__ o0, T* __restrict__ o1, long long total, long long R, int C) {
  struct alignas(sizeof(T) * VN) Vec { T v[VN]; };
  const int nvec = C / VN;
  const bool small = total < (1LL << 31);
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    long long gc;
    if (small) {
      const unsigned row = (unsigned)i / (unsigned)nvec, v = (unsigned)i - row * (unsigned)nvec;
      gc = (long long)(row / (unsigned)R) * C + v * VN;
    } else {
      const long long row = i / nvec;
      gc = (row / R) * C + (i - row * nvec) * VN;
    }
    const long long off = i * VN;
    const Vec a = *reinterpret_cast<const Vec*>(p0 + off);
    Vec r0, r1;
    if (!BWD) {
      const Vec w = *reinterpret_cast<const Vec*>(p1 + off);
#pragma unroll
      for (int e = 0; e < VN; ++e) {
        const float* k = coef + (gc + e) * 2;
        r0.v[e] = from_f32<T>(to_f32(a.v[e]) * k[0] + to_f32(w.v[e]) * k[1]);
      }
      *reinterpret_cast<Vec*>(o0 + off) = r0;
    } else {
#pragma unroll
      for (int e = 0; e < VN; ++e) {
        const float* k = coef + (gc + e) * 2;
        const float d = to_f32(a.v[e]), ad = add[gc + e];
        r0.v[e] = from_f32<T>(d * k[0] + ad);
        r1.v[e] = from_f32<T>(d * k[1] + ad);
      }
      *reinterpret_cast<Vec*>(o0 + off) = r0;
      *reinterpret_cast<Vec*>(o1 + off) = r1;
    }
  }
}

// ------------------------------------------------------------------------------------------------ SE MLP with a two-way softmax
// Mlp_cnn_shift.reweight on the pooled rows m (G, C), fp32: pre (G, Hd) = W1 m + b1;  z (G, 2C) = W2 gelu(pre) + b2;  out[g, c, :] =
// softmax(z[g, 2c], z[g, 2c + 1]).  The shape of the three-way kernels of tab_ops.hip (vmg_se_mlp_fwd / _bwd mode 1): one workgroup per pooled
// row forward; backward one launch for the rows (dz2, dz1 to the workspace, dm) and one for the parameters, which sums the rows in order.
__global__ __launch_bounds__(1024) void se2_fwd_kernel(const float* __restrict__ m, const float* __restrict__ w1, const float* __restrict__ b1,
                                                      const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ pre,
                                                      float* __restrict__ out, int C, int Hd) {
  extern __shared__ float sm[];
  float* mrow = sm;    // C
  float* z1 = sm + C;  // Hd
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nt = blockDim.x, nw = nt >> 6;
  for (int c = tid; c < C; c += nt) mrow[c] = m[(long long)g * C + c];
  __syncthreads();
  for (int j = wave; j < Hd; j += nw) {  // a wave per hidden unit: lanes stride over the C inputs
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += w1[(long long)j * C + c] * mrow[c];
    s = wave_sum(s) + (b1 ? b1[j] : 0.f);
    if (lane == 0) { pre[(long long)g * Hd + j] = s; z1[j] = gelu_erf(s); }
  }
  __syncthreads();
  for (int c = tid; c < C; c += nt) {
    float z[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int o = 2 * c + k;
      float s = b2 ? b2[o] : 0.f;
      const float* wr = w2 + (long long)o * Hd;
      for (int j = 0; j < Hd; ++j) s += wr[j] * z1[j];
      z[k] = s;
    }
    const float mx = fmaxf(z[0], z[1]);
    const float e0 = expf(z[0] - mx), e1 = expf(z[1] - mx), inv = 1.f / (e0 + e1);
    float* orow = out + ((long long)g * C + c) * 2;
    orow[0] = e0 * inv; orow[1] = e1 * inv;
  }
}

__global__ __launch_bounds__(1024) void se2_bwd_rows_kernel(const float* __restrict__ dout, const float* __restrict__ out, const float* __restrict__ pre,
                                                           const float* __restrict__ w1, const float* __restrict__ w2, float* __restrict__ dm,
                                                           float* __restrict__ ws, int G, int C, int Hd, float dm_scale) {
  extern __shared__ float sm[];
  const int Co = 2 * C;
  float* dz2 = sm;       // Co
  float* dz1 = sm + Co;  // Hd
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nt = blockDim.x, nw = nt >> 6;
  float* gz2 = ws + (long long)g * Co;
  float* gz1 = ws + (long long)G * Co + (long long)g * Hd;
  const float* orow = out + (long long)g * Co;
  const float* drow = dout + (long long)g * Co;
  for (int c = tid; c < C; c += nt) {  // softmax backward: dz_k = a_k (d_k - sum_j a_j d_j)
    const float a0 = orow[2 * c], a1 = orow[2 * c + 1], d0 = drow[2 * c], d1 = drow[2 * c + 1];
    const float sd = a0 * d0 + a1 * d1;
    const float v0 = a0 * (d0 - sd), v1 = a1 * (d1 - sd);
    dz2[2 * c] = v0; dz2[2 * c + 1] = v1;
    gz2[2 * c] = v0; gz2[2 * c + 1] = v1;
  }
  __syncthreads();
  for (int j = wave; j < Hd; j += nw) {
    float s = 0.f;
    for (int o = lane; o < Co; o += 64) s += dz2[o] * w2[(long long)o * Hd + j];
    s = wave_sum(s) * gelu_erf_grad(pre[(long long)g * Hd + j]);
    if (lane == 0) { dz1[j] = s; gz1[j] = s; }
  }
  __syncthreads();
  for (int c = tid; c < C; c += nt) {
    float s = 0.f;
    for (int j = 0; j < Hd; ++j) s += dz1[j] * w1[(long long)j * C + c];
    dm[(long long)g * C + c] = s * dm_scale;
  }
}

// one thread per element of dw1 (Hd, C), dw2 (2C, Hd), db1, db2, summing over the G rows in order
__global__ __launch_bounds__(256) void se2_bwd_params_kernel(const float* __restrict__ m, const float* __restrict__ pre, const float* __restrict__ ws,
                                                             float* __restrict__ dw1, float* __restrict__ db1, float* __restrict__ dw2,
                                                             float* __restrict__ db2, int G, int C, int Hd, int accumulate) {
  const int Co = 2 * C;
  const float* dz2 = ws;
  const float* dz1 = ws + (long long)G * Co;
  const int n1 = Hd * C, n2 = Co * Hd;
  const int i = blockIdx.x * 256 + threadIdx.x;
  float s = 0.f;
  if (i < n1) {
    const int j = i / C, c = i - j * C;
    for (int g = 0; g < G; ++g) s += dz1[g * Hd + j] * m[(long long)g * C + c];
    dw1[i] = accumulate ? dw1[i] + s : s;
  } else if (i < n1 + n2) {
    const int e = i - n1, o = e / Hd, j = e - o * Hd;
    for (int g = 0; g < G; ++g) s += dz2[(long long)g * Co + o] * gelu_erf(pre[g * Hd + j]);
    dw2[e] = accumulate ? dw2[e] + s : s;
  } else if (i < n1 + n2 + Hd) {
    const int j = i - n1 - n2;
    for (int g = 0; g < G; ++g) s += dz1[g * Hd + j];
    db1[j] = accumulate ? db1[j] + s : s;
  } else if (i < n1 + n2 + Hd + Co) {
    const int o = i - n1 - n2 - Hd;
    for (int g = 0; g < G; ++g) s += dz2[(long long)g * Co + o];
    db2[o] = accumulate ? db2[o] + s : s;
  }
}

template <typename T, int VN>
void patch_shift_launch(int mode, int blocks, hipStream_t st, const void* src, const void* xref, void* dst, long long total, int H, int W, int Cs, int g,
                        int sign) {
  if (mode == PS_COPY)
    hipLaunchKernelGGL((patch_shift_kernel<T, VN, PS_COPY>), dim3(blocks), dim3(256), 0, st, (const T*)src, (const T*)xref, (T*)dst, total, H, W, Cs, g, sign);
  else if (mode == PS_GELU_FWD)
    hipLaunchKernelGGL((patch_shift_kernel<T, VN, PS_GELU_FWD>), dim3(blocks), dim3(256), 0, st, (const T*)src, (const T*)xref, (T*)dst, total, H, W, Cs, g, sign);
  else
    hipLaunchKernelGGL((patch_shift_kernel<T, VN, PS_GELU_BWD>), dim3(blocks), dim3(256), 0, st, (const T*)src, (const T*)xref, (T*)dst, total, H, W, Cs, g, sign);
}

inline int grid_for(long long total) { return (int)(cdiv64(total, 256) > 8192 ? 8192 : cdiv64(total, 256)); }

}  // namespace

// The route of a patch-shift launch, a pure function of its arguments: VMG_SHIFT_VECTOR when the chunk width g = ceil(Cs / 9) and Cs are
// multiples of the 16-byte vector (8 bf16 / 4 fp32) and every pointer is 16-byte aligned, else VMG_SHIFT_ELEMENT.
extern "C" int vmg_patch_shift_plan(int dtype, int Cs, int aligned16) {
  if ((dtype != VMG_F32 && dtype != VMG_BF16) || Cs < 1) return -1;
  const int vn = dtype == VMG_BF16 ? 8 : 4;
  const int g = (Cs + 8) / 9;
  return (aligned16 && g % vn == 0 && Cs % vn == 0) ? VMG_SHIFT_VECTOR : VMG_SHIFT_ELEMENT;
}

static int patch_shift_dispatch(const char* who, int dtype, int sign, int mode, const void* src, const void* xref, void* dst, int N, int H, int W, int Cs,
                                void* stream) {
  VMG_CHECK(dtype == VMG_F32 || dtype == VMG_BF16, "%s: bad dtype", who);
  VMG_CHECK(sign == 1 || sign == -1, "%s: sign is +1 (shift) or -1 (shift_inv)", who);
  VMG_CHECK(src && dst && (xref || mode != PS_GELU_BWD), "%s: null pointer", who);
  VMG_CHECK(N >= 1 && H >= 1 && W >= 1 && Cs >= 1, "%s: N, H, W and Cs must be at least 1", who);
  const uintptr_t bits = (uintptr_t)src | (uintptr_t)dst | (mode == PS_GELU_BWD ? (uintptr_t)xref : 0);
  const int es = dtype == VMG_BF16 ? 2 : 4;
  VMG_CHECK(bits % es == 0, "%s: pointers must be aligned to the element size (%d bytes)", who, es);
  const int route = vmg_patch_shift_plan(dtype, Cs, bits % 16 == 0);
  const int vn = route == VMG_SHIFT_VECTOR ? 16 / es : 1;
  const int g = (Cs + 8) / 9;
  const long long total = (long long)N * H * W * (Cs / vn);
  const int blocks = grid_for(total);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VMG_BF16) {
    if (vn == 8) patch_shift_launch<bf16, 8>(mode, blocks, st, src, xref, dst, total, H, W, Cs, g, sign);
    else patch_shift_launch<bf16, 1>(mode, blocks, st, src, xref, dst, total, H, W, Cs, g, sign);
  } else {
    if (vn == 4) patch_shift_launch<float, 4>(mode, blocks, st, src, xref, dst, total, H, W, Cs, g, sign);
    else patch_shift_launch<float, 1>(mode, blocks, st, src, xref, dst, total, H, W, Cs, g, sign);
  }
  VMG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vmg_patch_shift_fwd(int dtype, int sign, int act, const void* x, void* y, int N, int H, int W, int Cs, void* stream) {
  VMG_CHECK(act == 0 || act == 3, "patch_shift_fwd: act is 0 (identity) or 3 (GELU)");
  return patch_shift_dispatch("patch_shift_fwd", dtype, sign, act == 3 ? PS_GELU_FWD : PS_COPY, x, nullptr, y, N, H, W, Cs, stream);
}

extern "C" int vmg_patch_shift_bwd(int dtype, int sign, int act, const void* dy, const void* x, void* dx, int N, int H, int W, int Cs, void* stream) {
  VMG_CHECK(act == 0 || act == 3, "patch_shift_bwd: act is 0 (identity) or 3 (GELU)");
  VMG_CHECK(sign == 1 || sign == -1, "patch_shift_bwd: sign is +1 (shift) or -1 (shift_inv)");
  // the adjoint of the shift with sign s is the shift with sign -s; the identity form is the forward's own instance
  return patch_shift_dispatch("patch_shift_bwd", dtype, -sign, act == 3 ? PS_GELU_BWD : PS_COPY, dy, x, dx, N, H, W, Cs, stream);
}

// vector width (elements) of the two-branch kernels: 16 bytes when C and the pointers allow, else 2 elements; 0: refuse
static int two_branch_vn(int dtype, int C, uintptr_t bits) {
  const int es = dtype == VMG_BF16 ? 2 : 4, vn = 16 / es;
  if (C % vn == 0 && bits % 16 == 0) return vn;
  if (C % 2 == 0 && bits % (2 * es) == 0) return 2;
  return 0;
}

extern "C" int vmg_group_reduce2(int dtype, const void* a, const void* b0, const void* b1, float* out, int G, int64_t R, int C, float scale, float* ws,
                                 int64_t ws_bytes, void* stream) {
  VMG_CHECK(dtype == VMG_F32 || dtype == VMG_BF16, "group_reduce2: bad dtype");
  VMG_CHECK(a && b0 && b1 && out && ws, "group_reduce2: null pointer");
  VMG_CHECK(G > 0 && R > 0 && C > 0 && C <= 512, "group_reduce2: bad arguments (G, R >= 1; 1 <= C <= 512)");
  const int vn = two_branch_vn(dtype, C, (uintptr_t)a | (uintptr_t)b0 | (uintptr_t)b1);
  VMG_CHECK(vn > 0 && C / vn <= 256, "group_reduce2: C must be even and the tensors aligned to two elements");
  VMG_CHECK(((uintptr_t)out | (uintptr_t)ws) % 4 == 0, "group_reduce2: out and ws must be 4-byte aligned");
  int chunks = 1024 / G;
  if (chunks < 1) chunks = 1;
  if (chunks > R / 64) chunks = (int)(R / 64 > 0 ? R / 64 : 1);
  VMG_CHECK((int64_t)G * chunks * C * 2 * (int64_t)sizeof(float) <= ws_bytes, "group_reduce2: workspace too small (vmg_group_reduce_ws_bytes)");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(G * chunks), blk(256);
  if (dtype == VMG_BF16) {
    if (vn == 8) hipLaunchKernelGGL((reduce2_kernel<bf16, 8>), grid, blk, 0, st, (const bf16*)a, (const bf16*)b0, (const bf16*)b1, ws, (long long)R, C, chunks);
    else hipLaunchKernelGGL((reduce2_kernel<bf16, 2>), grid, blk, 0, st, (const bf16*)a, (const bf16*)b0, (const bf16*)b1, ws, (long long)R, C, chunks);
  } else {
    if (vn == 4) hipLaunchKernelGGL((reduce2_kernel<float, 4>), grid, blk, 0, st, (const float*)a, (const float*)b0, (const float*)b1, ws, (long long)R, C, chunks);
    else hipLaunchKernelGGL((reduce2_kernel<float, 2>), grid, blk, 0, st, (const float*)a, (const float*)b0, (const float*)b1, ws, (long long)R, C, chunks);
  }
  VMG_LAUNCH_CHECK();
  hipLaunchKernelGGL(reduce2_final_kernel, dim3(G * cdiv(2 * C, 16)), dim3(256), 0, st, (const float*)ws, out, chunks, 2 * C, scale);
  VMG_LAUNCH_CHECK();
  return 0;
}

static int mix2_dispatch(const char* who, int dtype, bool bwd, const void* p0, const void* p1, const float* coef, const float* add, void* o0, void* o1,
                         int64_t rows, int64_t R, int C, void* stream) {
  VMG_CHECK(dtype == VMG_F32 || dtype == VMG_BF16, "%s: bad dtype", who);
  VMG_CHECK(p0 && o0 && coef && (bwd ? (add && o1) : p1 != nullptr), "%s: null pointer", who);
  VMG_CHECK(rows > 0 && R > 0 && rows % R == 0 && C > 0, "%s: %lld rows do not split into groups of %lld (C >= 1)", who, (long long)rows, (long long)R);
  const int vn = two_branch_vn(dtype, C, (uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)o0 | (uintptr_t)o1);
  VMG_CHECK(vn > 0, "%s: C must be even and the tensors aligned to two elements", who);
  VMG_CHECK(((uintptr_t)coef | (uintptr_t)add) % 4 == 0, "%s: coefficients must be 4-byte aligned", who);
  const long long total = (long long)rows * (C / vn);
  const int blocks = grid_for(total);
  hipStream_t st = (hipStream_t)stream;
#define VMG_MIX2(T_, VN_)                                                                                                                             \
  do {                                                                                                                                                \
    if (bwd) hipLaunchKernelGGL((mix2_kernel<T_, VN_, true>), dim3(blocks), dim3(256), 0, st, (const T_*)p0, (const T_*)p1, coef, add, (T_*)o0, (T_*)o1, \
                                total, (long long)R, C);                                                                                              \
    else hipLaunchKernelGGL((mix2_kernel<T_, VN_, false>), dim3(blocks), dim3(256), 0, st, (const T_*)p0, (const T_*)p1, coef, add, (T_*)o0, (T_*)o1,    \
                            total, (long long)R, C);                                                                                                  \
  } while (0)
  if (dtype == VMG_BF16) {
    if (vn == 8) VMG_MIX2(bf16, 8);
    else VMG_MIX2(bf16, 2);
  } else {
    if (vn == 4) VMG_MIX2(float, 4);
    else VMG_MIX2(float, 2);
  }
#undef VMG_MIX2
  VMG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vmg_mix2_fwd(int dtype, const void* h, const void* w, const float* coef, void* y, int64_t rows, int64_t R, int C, void* stream) {
  return mix2_dispatch("mix2_fwd", dtype, false, h, w, coef, nullptr, y, nullptr, rows, R, C, stream);
}

extern "C" int vmg_mix2_bwd(int dtype, const void* dy, const float* coef, const float* add, void* dh, void* dw, int64_t rows, int64_t R, int C,
                            void* stream) {
  return mix2_dispatch("mix2_bwd", dtype, true, dy, nullptr, coef, add, dh, dw, rows, R, C, stream);
}

extern "C" int vmg_se_mlp2_fwd(const float* m, const float* w1, const float* b1, const float* w2, const float* b2, float* pre, float* out, int G, int C,
                               int Hd, void* stream) {
  VMG_CHECK(m && w1 && w2 && pre && out, "se_mlp2_fwd: null pointer");
  VMG_CHECK(G > 0 && C > 0 && Hd > 0, "se_mlp2_fwd: G, C and Hd must be at least 1");
  VMG_CHECK(((uintptr_t)m | (uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)w2 | (uintptr_t)b2 | (uintptr_t)pre | (uintptr_t)out) % 4 == 0,
            "se_mlp2_fwd: pointers must be 4-byte aligned");
  VMG_CHECK((C + Hd) * 4LL <= 64 * 1024, "se_mlp2_fwd: C + Hd too large");
  hipLaunchKernelGGL(se2_fwd_kernel, dim3(G), dim3(1024), (C + Hd) * 4, (hipStream_t)stream, m, w1, b1, w2, b2, pre, out, C, Hd);
  VMG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vmg_se_mlp2_bwd(const float* dout, const float* out, const float* m, const float* pre, const float* w1, const float* w2, float* dm,
                               float* dw1, float* db1, float* dw2, float* db2, float* ws, int G, int C, int Hd, float dm_scale, int accumulate,
                               void* stream) {
  VMG_CHECK(dout && out && m && pre && w1 && w2 && dm && dw1 && db1 && dw2 && db2 && ws, "se_mlp2_bwd: null pointer");
  VMG_CHECK(G > 0 && C > 0 && Hd > 0, "se_mlp2_bwd: G, C and Hd must be at least 1");
  VMG_CHECK(((uintptr_t)dout | (uintptr_t)out | (uintptr_t)m | (uintptr_t)pre | (uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)dm | (uintptr_t)dw1 | (uintptr_t)db1 |
             (uintptr_t)dw2 | (uintptr_t)db2 | (uintptr_t)ws) % 4 == 0, "se_mlp2_bwd: pointers must be 4-byte aligned");
  VMG_CHECK((2 * C + Hd) * 4LL <= 64 * 1024, "se_mlp2_bwd: 2 C + Hd too large");
  hipLaunchKernelGGL(se2_bwd_rows_kernel, dim3(G), dim3(1024), (2 * C + Hd) * 4, (hipStream_t)stream, dout, out, pre, w1, w2, dm, ws, G, C, Hd, dm_scale);
  VMG_LAUNCH_CHECK();
  const int total = Hd * C + 2 * C * Hd + Hd + 2 * C;
  hipLaunchKernelGGL(se2_bwd_params_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, m, pre, (const float*)ws, dw1, db1, dw2, db2, G, C, Hd,
                     accumulate);
  VMG_LAUNCH_CHECK();
  return 0;
}
