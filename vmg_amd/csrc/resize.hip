// LR frames from HR frames (reference: datasets/generate_LR.py:32-37 with utils/image_resize.py imresize_np(img, 1 / s, True)): the
// MATLAB-imresize antialiased bicubic downscale of T uint8 frames by an integer factor s in {2, 3, 4}, one launch.
//   bicubic_down_kernel<S>   a workgroup owns a 16 x 16 tile of LR pixels, all three channels.  It stages the 19S rows x 19S pixels of HR bytes
//                            the tile reaches (4S taps per axis, border indices mirrored with edge repeat at fetch time) in LDS, exactly as
//                            the rows lie in memory: three runs of pixels for planar frames, one run of interleaved bytes otherwise, so that
//                            aligned rows are fetched as dwords.  Then the vertical pass: one thread per staged byte column slides down
//                            the rows and leaves 16 float64 sums; the horizontal pass: one thread per LR pixel, 4S taps per channel from
//                            that strip; the results cross LDS once more so that the store runs along the output rows.
// Both passes accumulate in float64 in a fixed order (tap 0 first), nothing is added across threads: two calls give the same bits.
// For an integer S the normalised tap weights are the same for every output sample: one table of 4S doubles, computed on the host.
#include <math.h>

#include "common.h"

namespace {

constexpr int TILE = 16;  // LR pixels per tile edge

struct LrView {
  const unsigned char* p;
  long long sf, sc, sr, sp;  // element strides: frame, channel, row, pixel
};
struct LrTaps {
  double w[16];  // 4S normalised weights, tap q reads input index o*S + off + q
};

enum { LR_BYTES = 0, LR_PLANAR_DWORDS = 1, LR_INTER_DWORDS = 2 };  // how the patch is fetched and laid out

template <int S>
struct Geo {
  static constexpr int NT = 4 * S;                     // taps per axis (the reference's P = 4S + 2 without its two zero ends)
  static constexpr int PH = (TILE - 1) * S + NT;       // staged rows, and pixels per row
  static constexpr int PWA = (PH + 3 + 3) / 4 * 4;     // pixels per channel run, with room for a start 3 bytes before the first pixel
  static constexpr int ROWB = 3 * PWA;                 // staged bytes per row (<= 240)
  static constexpr int PITCH = ROWB + 1;               // doubles per strip row (odd: the horizontal pass reads down the strip rows)
};

// index of a sample outside [0, n): mirrored with edge repeat (-1 -> 0, n -> n - 1); the clamp only matters for the columns of a partial
// tile that lie wholly outside the frame, whose results are never stored
__device__ __forceinline__ int mirror(int i, int n) {
  if (i < 0) i = -i - 1;
  if (i >= n) i = 2 * n - 1 - i;
  return min(max(i, 0), n - 1);
}

template <int S>
__device__ __forceinline__ void stage_patch(unsigned char* patch, const LrView& v, int mode, int mis, int f, int gy0, int gx0, int H, int W,
                                            int* kbase) {
  using G = Geo<S>;
  const unsigned char* base = v.p + (long long)f * v.sf;
  if (mode == LR_INTER_DWORDS) {
    // a row is one run of 3W bytes; byte b of the run is channel b % 3 of pixel b / 3.  b0 + mis is a multiple of 4.
    const int b0 = (((3 * gx0 + mis) >> 2) << 2) - mis;
    *kbase = 3 * gx0 - b0;
    for (int i = threadIdx.x; i < G::PH * (G::ROWB / 4); i += 256) {
      const int r = i / (G::ROWB / 4), d = i % (G::ROWB / 4);
      const unsigned char* row = base + (long long)mirror(gy0 + r, H) * v.sr;
      const int b = b0 + 4 * d;
      unsigned int word;
      if (b >= 0 && b + 3 < 3 * W) {
        word = *reinterpret_cast<const unsigned int*>(row + b);
      } else {
        word = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int bb = b + q;
          const int gx = bb >= 0 ? bb / 3 : -((2 - bb) / 3);
          word |= (unsigned int)row[3 * mirror(gx, W) + (bb - 3 * gx)] << (8 * q);
        }
      }
      *reinterpret_cast<unsigned int*>(patch + r * G::ROWB + 4 * d) = word;
    }
    return;
  }
  // three runs of PWA pixels per row, one per channel; pixel a0 + xx of the frame lies at byte xx of its run
  const int a0 = mode == LR_PLANAR_DWORDS ? (((gx0 + mis) >> 2) << 2) - mis : gx0;
  *kbase = gx0 - a0;
  if (mode == LR_PLANAR_DWORDS) {
    for (int i = threadIdx.x; i < G::PH * (G::ROWB / 4); i += 256) {
      const int d = i % (G::PWA / 4), c = (i / (G::PWA / 4)) % 3, r = i / (G::ROWB / 4);
      const unsigned char* row = base + c * v.sc + (long long)mirror(gy0 + r, H) * v.sr;
      const int gx = a0 + 4 * d;
      unsigned int word;
      if (gx >= 0 && gx + 3 < W) {
        word = *reinterpret_cast<const unsigned int*>(row + gx);
      } else {
        word = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) word |= (unsigned int)row[mirror(gx + q, W)] << (8 * q);
      }
      *reinterpret_cast<unsigned int*>(patch + r * G::ROWB + c * G::PWA + 4 * d) = word;
    }
    return;
  }
  // any strides, byte by byte; consecutive lanes follow the layout's fastest axis
  const bool ch_fast = v.sc < v.sp;
  for (int i = threadIdx.x; i < G::PH * G::ROWB; i += 256) {
    const int r = i / G::ROWB, k = i % G::ROWB;
    const int c = ch_fast ? k % 3 : k / G::PWA, xx = ch_fast ? k / 3 : k % G::PWA;
    patch[r * G::ROWB + c * G::PWA + xx] = base[c * v.sc + (long long)mirror(gy0 + r, H) * v.sr + (long long)mirror(a0 + xx, W) * v.sp];
  }
}

__device__ __forceinline__ void store_lr(void* out, int out_type, long long idx, double v) {
  if (out_type == VMG_LR_F64) {
    static_cast<double*>(out)[idx] = v;
    return;
  }
  const double q = fmin(255.0, fmax(0.0, rint(v)));  // round half to even, then the clamp of a uint8 store
  if (out_type == VMG_LR_U8) {
    static_cast<unsigned char*>(out)[idx] = (unsigned char)(int)q;
    return;
  }
  const float x = __fdiv_rn((float)q, 255.0f);  // the correctly rounded quotient, as u8.float().div(255)
  if (out_type == VMG_LR_F32)
    static_cast<float*>(out)[idx] = x;
  else
    static_cast<bf16*>(out)[idx] = (bf16)x;
}

template <int S>
__global__ __launch_bounds__(256) void bicubic_down_kernel(LrView in, int mode, int mis, int H, int W, int off, LrTaps taps, int out_type,
                                                           void* __restrict__ out) {
  using G = Geo<S>;
  constexpr int RES_BYTES = 3 * TILE * TILE * (int)sizeof(double);  // the tile's results reuse the patch
  __shared__ __attribute__((aligned(8))) unsigned char patch[G::PH * G::ROWB > RES_BYTES ? G::PH * G::ROWB : RES_BYTES];
  __shared__ double strip[TILE * G::PITCH];
  static_assert(G::ROWB <= 256, "one thread per staged byte column");

  const int tid = threadIdx.x;
  const int oh = H / S, ow = W / S;
  const int ox0 = blockIdx.x * TILE, oy0 = blockIdx.y * TILE, f = blockIdx.z;
  int kbase;
  stage_patch<S>(patch, in, mode, mis, f, oy0 * S + off, ox0 * S + off, H, W, &kbase);
  __syncthreads();

  // vertical: staged row r is tap r - o*S of output row o
  if (tid < G::ROWB) {
    double acc[TILE];
#pragma unroll
    for (int o = 0; o < TILE; ++o) acc[o] = 0.0;
#pragma unroll
    for (int r = 0; r < G::PH; ++r) {
      const double v = (double)patch[r * G::ROWB + tid];
#pragma unroll
      for (int o = 0; o < TILE; ++o) {
        const int q = r - o * S;
        if (q >= 0 && q < G::NT) acc[o] += taps.w[q] * v;
      }
    }
#pragma unroll
    for (int o = 0; o < TILE; ++o) strip[o * G::PITCH + tid] = acc[o];
  }
  __syncthreads();

  // horizontal: consecutive lanes take consecutive output rows (strip rows: an odd pitch apart)
  double* res = reinterpret_cast<double*>(patch);
  {
    const int oy = tid & (TILE - 1), ox = tid >> 4;
    const bool inter = mode == LR_INTER_DWORDS;
    const int kc = inter ? 1 : G::PWA, kx = inter ? 3 : 1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double* s = strip + oy * G::PITCH + kbase + c * kc + ox * S * kx;
      double acc = 0.0;
#pragma unroll
      for (int q = 0; q < G::NT; ++q) acc += taps.w[q] * s[q * kx];
      res[(c * TILE + oy) * TILE + ox] = acc;
    }
  }
  __syncthreads();

  {
    const int oy = tid >> 4, ox = tid & (TILE - 1);
    if (oy0 + oy < oh && ox0 + ox < ow) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        store_lr(out, out_type, (((long long)f * 3 + c) * oh + oy0 + oy) * ow + ox0 + ox, res[(c * TILE + oy) * TILE + ox]);
    }
  }
}

// Keys' cubic, a = -0.5
double keys_cubic(double x) {
  x = fabs(x);
  if (x <= 1.0) return 1.5 * x * x * x - 2.5 * x * x + 1.0;
  if (x <= 2.0) return -0.5 * x * x * x + 2.5 * x * x - 4.0 * x + 2.0;
  return 0.0;
}

}  // namespace

extern "C" int vmg_bicubic_down(const unsigned char* src, const int64_t* strides, int T, int H, int W, int scale, int out_type, void* out,
                                void* stream) {
  VMG_CHECK(scale >= 2 && scale <= 4, "bicubic_down: scale must be 2, 3 or 4, got %d", scale);
  VMG_CHECK(T >= 1 && T <= 65535, "bicubic_down: 1 to 65535 frames per call, got %d", T);
  VMG_CHECK(H > 0 && W > 0 && H % scale == 0 && W % scale == 0, "bicubic_down: a %d x %d frame is no multiple of the scale %d (crop it first)", H, W,
            scale);
  VMG_CHECK(H >= 4 * scale && W >= 4 * scale, "bicubic_down: a %d x %d frame is smaller than the %d-pixel support of the filter", H, W, 4 * scale);
  VMG_CHECK(H <= (1 << 16) && W <= (1 << 16), "bicubic_down: frame too large");
  VMG_CHECK(out_type >= VMG_LR_U8 && out_type <= VMG_LR_F64, "bicubic_down: unknown output type %d", out_type);
  VMG_CHECK(src && strides && out, "bicubic_down: null argument");
  const int esize = out_type == VMG_LR_U8 ? 1 : out_type == VMG_LR_BF16 ? 2 : out_type == VMG_LR_F32 ? 4 : 8;
  VMG_CHECK(((uintptr_t)out & (esize - 1)) == 0, "bicubic_down: misaligned output");
  for (int i = 0; i < 4; ++i) VMG_CHECK(strides[i] >= 0, "bicubic_down: negative stride");
  LrView in{src, strides[0], strides[1], strides[2], strides[3]};

  // output sample o sits at the 1-based input coordinate u = (o + 1) s + 0.5 (1 - s); its first sample with a non-zero weight is the
  // 1-based floor(u - 2s) + 1, the 0-based o*s + off
  const double s = (double)scale, u0 = s + 0.5 * (1.0 - s);
  const int off = (int)floor(u0 - 2.0 * s);
  LrTaps taps;
  double sum = 0.0;
  for (int q = 0; q < 16; ++q) {
    taps.w[q] = q < 4 * scale ? keys_cubic((u0 - (double)(off + q + 1)) / s) : 0.0;
    sum += taps.w[q];
  }
  for (int q = 0; q < 16; ++q) taps.w[q] /= sum;

  // rows whose starts differ by multiples of 4 bytes are fetched as dwords, whatever the start itself is
  const int mis = (int)((uintptr_t)src & 3);
  const bool rows4 = in.sf % 4 == 0 && in.sr % 4 == 0;
  int mode = LR_BYTES;
  if (rows4 && in.sp == 1 && in.sc % 4 == 0) mode = LR_PLANAR_DWORDS;
  if (rows4 && in.sp == 3 && in.sc == 1) mode = LR_INTER_DWORDS;

  const dim3 grid(cdiv(W / scale, TILE), cdiv(H / scale, TILE), T);
  hipStream_t st = (hipStream_t)stream;
  if (scale == 2)
    hipLaunchKernelGGL(bicubic_down_kernel<2>, grid, dim3(256), 0, st, in, mode, mis, H, W, off, taps, out_type, out);
  else if (scale == 3)
    hipLaunchKernelGGL(bicubic_down_kernel<3>, grid, dim3(256), 0, st, in, mode, mis, H, W, off, taps, out_type, out);
  else
    hipLaunchKernelGGL(bicubic_down_kernel<4>, grid, dim3(256), 0, st, in, mode, mis, H, W, off, taps, out_type, out);
  VMG_LAUNCH_CHECK();
  return 0;
}
