// Best window per frame for REDS evaluation (reference: tools/Tester.py:180-213, Tester.test_clips_max): every temporal window is scored frame
// by frame against HR, and a frame keeps the window that scored best.  Streamed: one window at a time, one canvas, no score leaves the card.
//   frame_sqerr_planar_kernel / frame_sqerr_u8_kernel   a FIXED number of workgroups per frame (a function of the frame size alone) walk the frame
//                               with a grid stride; each thread adds (clamp(out) - clamp(hr))^2 in float64, the sums are reduced by wavefront
//                               shuffles, then across the four wavefronts through LDS, and leave as one float64 partial per workgroup.
//   frame_sqerr_final_kernel    one thread per frame adds that frame's partials in index order and divides by the element count.
//   best_window_select_kernel   per frame of the clip: the float32 score from the error, the decision (window 0 always, later windows only on a
//                               STRICTLY higher score: torch.max's first maximum over a table whose uncovered entries are 0), the copy of a
//                               winning frame into its canvas slot as fp32, and best / choice carried from the *_in to the *_out arrays.
// No atomics, no memset, no allocation: equal inputs give equal bits.
#include "common.h"

namespace {

constexpr int BW_THREADS = 256;
constexpr int BW_MAX_BPF = 64;             // workgroups per frame, at most
constexpr long long BW_BLOCK_ELEMS = 4096;  // elements a workgroup should at least have before another one is added

int blocks_per_frame(long long elems) {
  const long long b = (elems + BW_BLOCK_ELEMS - 1) / BW_BLOCK_ELEMS;
  return (int)(b < 1 ? 1 : (b > BW_MAX_BPF ? BW_MAX_BPF : b));
}

// torch's clamp(0, 1): a NaN stays a NaN
__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

__device__ __forceinline__ double sq_diff(float a, float b) {
  const double d = (double)a - (double)b;
  return d * d;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the workgroup's sum -> *dst (thread 0 adds the four wavefront sums in wavefront order)
__device__ __forceinline__ void block_sum_store(double acc, double* dst) {
  __shared__ double red[BW_THREADS / 64];
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = red[0];
#pragma unroll
    for (int w = 1; w < BW_THREADS / 64; ++w) s += red[w];
    *dst = s;
  }
}

// out and hr both planar: the frame is a flat run of E elements on both sides
template <typename TO, typename TH>
__global__ __launch_bounds__(BW_THREADS) void frame_sqerr_planar_kernel(const TO* __restrict__ out, long long out_fs, const TH* __restrict__ hr,
                                                                        long long hr_fs, long long E, int vec_ok, double* __restrict__ ws) {
  const int f = blockIdx.y;
  const TO* o = out + (long long)f * out_fs;
  const TH* h = hr + (long long)f * hr_fs;
  const long long stride = (long long)gridDim.x * BW_THREADS;
  const long long i0 = (long long)blockIdx.x * BW_THREADS + threadIdx.x;
  double acc = 0.0;
  long long done = 0;
  if (vec_ok) {
    const long long nv = E >> 2;
    for (long long v = i0; v < nv; v += stride) {
      float a[4], b[4];
      load4(o + 4 * v, a);
      load4(h + 4 * v, b);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc += sq_diff(clamp01(a[k]), clamp01(b[k]));
    }
    done = nv << 2;
  }
  for (long long i = done + i0; i < E; i += stride) acc += sq_diff(clamp01(to_f32(o[i])), clamp01(to_f32(h[i])));
  block_sum_store(acc, ws + (long long)f * gridDim.x + blockIdx.x);
}

struct U8x12 {
  uint32_t w[3];
};

// out planar (3, P pixels), hr interleaved bytes (P, 3): four pixels per thread and step = three 16-byte (fp32) loads and one 12-byte load
template <typename TO>
__global__ __launch_bounds__(BW_THREADS) void frame_sqerr_u8_kernel(const TO* __restrict__ out, long long out_fs, const unsigned char* __restrict__ hr,
                                                                    long long hr_fs, long long P, int vec_ok, double* __restrict__ ws) {
  const int f = blockIdx.y;
  const TO* o = out + (long long)f * out_fs;
  const unsigned char* h = hr + (long long)f * hr_fs;
  const long long stride = (long long)gridDim.x * BW_THREADS;
  const long long i0 = (long long)blockIdx.x * BW_THREADS + threadIdx.x;
  double acc = 0.0;
  long long done = 0;
  if (vec_ok) {
    const long long nv = P >> 2;
    for (long long v = i0; v < nv; v += stride) {
      const U8x12 raw = *reinterpret_cast<const U8x12*>(h + 12 * v);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float a[4];
        load4(o + c * P + 4 * v, a);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int byte_idx = 3 * k + c;
          const uint32_t b = (raw.w[byte_idx >> 2] >> (8 * (byte_idx & 3))) & 0xffu;
          // Tester.evaluate: HR.astype(np.float32) / 255. -- the correctly rounded quotient; it lies in [0, 1], a clamp changes nothing
          acc += sq_diff(clamp01(a[k]), __fdiv_rn((float)b, 255.0f));
        }
      }
    }
    done = nv << 2;
  }
  for (long long p = done + i0; p < P; p += stride) {
#pragma unroll
    for (int c = 0; c < 3; ++c) acc += sq_diff(clamp01(to_f32(o[c * P + p])), __fdiv_rn((float)h[3 * p + c], 255.0f));
  }
  block_sum_store(acc, ws + (long long)f * gridDim.x + blockIdx.x);
}

__global__ __launch_bounds__(64) void frame_sqerr_final_kernel(const double* __restrict__ ws, int bpf, int n, double count, double* __restrict__ err) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= n) return;
  const double* p = ws + (long long)f * bpf;
  double s = p[0];
  for (int i = 1; i < bpf; ++i) s += p[i];
  err[f] = s / count;
}

template <typename T>
struct Vec16;
template <>
struct Vec16<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void copy(const float* s, float* d) { *reinterpret_cast<float4*>(d) = *reinterpret_cast<const float4*>(s); }
};
template <>
struct Vec16<bf16> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void copy(const bf16* s, float* d) {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(s);
    *reinterpret_cast<float4*>(d) = make_float4((float)t[0], (float)t[1], (float)t[2], (float)t[3]);
    *reinterpret_cast<float4*>(d + 4) = make_float4((float)t[4], (float)t[5], (float)t[6], (float)t[7]);
  }
};

// grid (workgroups per frame, T).  Every workgroup of a frame reads err[i] and best_in[t] and so takes the same decision; workgroup 0 of the
// frame writes best_out / choice_out / table.  Frames outside [t0, t0 + n) only carry best and choice over.
template <typename T>
__global__ __launch_bounds__(BW_THREADS) void best_window_select_kernel(const T* __restrict__ out, long long out_fs, const double* __restrict__ err, int n,
                                                                        long long E, int t0, int window, float cap, float* __restrict__ canvas,
                                                                        const float* __restrict__ best_in, const int* __restrict__ choice_in,
                                                                        float* __restrict__ best_out, int* __restrict__ choice_out,
                                                                        float* __restrict__ table, int n_windows) {
  const int t = blockIdx.y, i = t - t0;
  const bool covered = i >= 0 && i < n;
  const float prev = best_in[t];
  float psnr = 0.0f;
  bool take = false;
  if (covered) {
    const double e = err[i];
    psnr = (float)(e == 0.0 ? (double)cap : 10.0 * log10(1.0 / e));  // the reference keeps its scores in a float32 table and compares them there
    take = window == 0 || psnr > prev;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    best_out[t] = take ? psnr : prev;
    choice_out[t] = take ? window : choice_in[t];
    if (covered && table) table[(long long)t * n_windows + window] = psnr;
  }
  if (!take) return;
  const T* s = out + (long long)i * out_fs;
  float* d = canvas + (long long)t * E;
  const long long stride = (long long)gridDim.x * BW_THREADS;
  const long long i0 = (long long)blockIdx.x * BW_THREADS + threadIdx.x;
  constexpr int V = Vec16<T>::N;
  // elements in front of the first 16-byte boundary of the source; the vector body needs the canvas at a 16-byte boundary there too
  long long head = (long long)(((16 - (int)((uintptr_t)s & 15)) & 15) / (int)sizeof(T));
  if (head > E) head = E;
  long long nv = 0;
  if ((((uintptr_t)(d + head)) & 15) == 0) {
    nv = (E - head) / V;
  } else {
    head = 0;
  }
  for (long long v = i0; v < nv; v += stride) Vec16<T>::copy(s + head + v * V, d + head + v * V);
  // what the vectors leave: the head, then the tail
  const long long rest = E - nv * V;
  for (long long r = i0; r < rest; r += stride) {
    const long long j = r < head ? r : r + nv * V;
    d[j] = to_f32(s[j]);
  }
}

bool aligned_to(const void* p, int bytes) { return ((uintptr_t)p % (uintptr_t)bytes) == 0; }

}  // namespace

extern "C" int64_t vmg_frame_sqerr_ws_bytes(int n, int C, int h, int w) {
  if (n < 1 || C < 1 || h < 1 || w < 1) return 0;
  return (int64_t)n * blocks_per_frame((long long)C * h * w) * (int64_t)sizeof(double);
}

extern "C" int vmg_frame_sqerr(int out_dtype, const void* out, int64_t out_fs, int hr_type, const void* hr, int64_t hr_fs, int n, int C, int h, int w,
                               void* ws, int64_t ws_bytes, double* err, void* stream) {
  VMG_CHECK(out && hr && ws && err, "frame_sqerr: null argument");
  VMG_CHECK(n >= 1 && n <= 65535, "frame_sqerr: 1 to 65535 frames per call, got %d", n);
  VMG_CHECK(C >= 1 && h >= 1 && w >= 1, "frame_sqerr: empty frame (%d, %d, %d)", C, h, w);
  VMG_CHECK(out_dtype == 0 || out_dtype == 1, "frame_sqerr: out must be fp32 (0) or bf16 (1), got %d", out_dtype);
  VMG_CHECK(hr_type == VMG_HR_F32 || hr_type == VMG_HR_BF16 || hr_type == VMG_HR_U8, "frame_sqerr: unknown hr type %d", hr_type);
  VMG_CHECK(hr_type != VMG_HR_U8 || C == 3, "frame_sqerr: interleaved uint8 frames have 3 channels, out has %d", C);
  const long long E = (long long)C * h * w, P = (long long)h * w;
  VMG_CHECK(out_fs >= 0 && hr_fs >= 0 && (n == 1 || (out_fs >= E && hr_fs >= E)), "frame_sqerr: frame strides must be at least one frame (%lld elements)", E);
  VMG_CHECK(ws_bytes >= vmg_frame_sqerr_ws_bytes(n, C, h, w), "frame_sqerr: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
            (long long)vmg_frame_sqerr_ws_bytes(n, C, h, w));
  VMG_CHECK(aligned_to(ws, 8) && aligned_to(err, 8), "frame_sqerr: workspace and err must be 8-byte aligned");
  const int osz = out_dtype == 0 ? 4 : 2;
  VMG_CHECK(aligned_to(out, osz), "frame_sqerr: out is not aligned to its element");
  VMG_CHECK(hr_type == VMG_HR_U8 || aligned_to(hr, hr_type == VMG_HR_F32 ? 4 : 2), "frame_sqerr: hr is not aligned to its element");
  const int bpf = blocks_per_frame(E);
  const dim3 grid(bpf, n);
  hipStream_t st = (hipStream_t)stream;
  double* wsd = (double*)ws;
  // four elements per load on both sides: every frame must start at such a boundary
  const bool out_vec = aligned_to(out, 4 * osz) && (n == 1 || out_fs % 4 == 0);
  if (hr_type == VMG_HR_U8) {
    const int vec_ok = out_vec && P % 4 == 0 && aligned_to(hr, 4) && (n == 1 || hr_fs % 4 == 0);
    if (out_dtype == 0)
      hipLaunchKernelGGL(frame_sqerr_u8_kernel<float>, grid, dim3(BW_THREADS), 0, st, (const float*)out, (long long)out_fs, (const unsigned char*)hr,
                         (long long)hr_fs, P, vec_ok, wsd);
    else
      hipLaunchKernelGGL(frame_sqerr_u8_kernel<bf16>, grid, dim3(BW_THREADS), 0, st, (const bf16*)out, (long long)out_fs, (const unsigned char*)hr,
                         (long long)hr_fs, P, vec_ok, wsd);
  } else {
    const int hsz = hr_type == VMG_HR_F32 ? 4 : 2;
    const int vec_ok = out_vec && aligned_to(hr, 4 * hsz) && (n == 1 || hr_fs % 4 == 0);
#define VMG_SQERR_PLANAR(TO, TH)                                                                                                                       \
  hipLaunchKernelGGL((frame_sqerr_planar_kernel<TO, TH>), grid, dim3(BW_THREADS), 0, st, (const TO*)out, (long long)out_fs, (const TH*)hr, (long long)hr_fs, \
                     E, vec_ok, wsd)
    if (out_dtype == 0 && hr_type == VMG_HR_F32) VMG_SQERR_PLANAR(float, float);
    else if (out_dtype == 0) VMG_SQERR_PLANAR(float, bf16);
    else if (hr_type == VMG_HR_F32) VMG_SQERR_PLANAR(bf16, float);
    else VMG_SQERR_PLANAR(bf16, bf16);
#undef VMG_SQERR_PLANAR
  }
  VMG_LAUNCH_CHECK();
  hipLaunchKernelGGL(frame_sqerr_final_kernel, dim3(cdiv(n, 64)), dim3(64), 0, st, (const double*)wsd, bpf, n, (double)E, err);
  VMG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vmg_best_window_select(int dtype, const void* out, int64_t out_fs, const double* err, int n, int64_t frame_elems, int T, int t0, int window,
                                      float cap, float* canvas, const float* best_in, const int* choice_in, float* best_out, int* choice_out,
                                      float* table, int n_windows, void* stream) {
  VMG_CHECK(out && err && canvas && best_in && choice_in && best_out && choice_out, "best_window_select: null argument");
  VMG_CHECK(dtype == 0 || dtype == 1, "best_window_select: out must be fp32 (0) or bf16 (1), got %d", dtype);
  VMG_CHECK(T >= 1 && T <= 65535, "best_window_select: 1 to 65535 frames, got %d", T);
  VMG_CHECK(n >= 1 && t0 >= 0 && (long long)t0 + n <= T, "best_window_select: window [%d, %d + %d) leaves the %d frames", t0, t0, n, T);
  VMG_CHECK(frame_elems >= 1, "best_window_select: empty frame");
  VMG_CHECK(out_fs >= 0 && (n == 1 || out_fs >= frame_elems), "best_window_select: the frame stride must be at least one frame");
  VMG_CHECK(n_windows >= 1 && window >= 0 && window < n_windows, "best_window_select: window index %d of %d", window, n_windows);
  VMG_CHECK(best_in != best_out && choice_in != choice_out, "best_window_select: best / choice are ping-ponged, *_in and *_out must differ");
  VMG_CHECK(aligned_to(out, dtype == 0 ? 4 : 2) && aligned_to(canvas, 4) && aligned_to(err, 8), "best_window_select: misaligned argument");
  const dim3 grid(blocks_per_frame(frame_elems), T);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0)
    hipLaunchKernelGGL(best_window_select_kernel<float>, grid, dim3(BW_THREADS), 0, st, (const float*)out, (long long)out_fs, err, n, (long long)frame_elems,
                       t0, window, cap, canvas, best_in, choice_in, best_out, choice_out, table, n_windows);
  else
    hipLaunchKernelGGL(best_window_select_kernel<bf16>, grid, dim3(BW_THREADS), 0, st, (const bf16*)out, (long long)out_fs, err, n, (long long)frame_elems, t0,
                       window, cap, canvas, best_in, choice_in, best_out, choice_out, table, n_windows);
  VMG_LAUNCH_CHECK();
  return 0;
}
