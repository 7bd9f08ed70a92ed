// Frame scoring (reference: tools/test_reds4.py:194-283 with utils/metrics.py:11-70): PSNR, PSNR-Y, SSIM and SSIM-Y sums of T uint8
// frame pairs from ONE launch, plus a small ordered reduction.
//   frame_metrics_tile_kernel   a workgroup owns a 16 x 32 tile of one frame pair.  It stages the tile and a 10-pixel halo (the 11-tap
//                               window reaches 5 pixels each way; the "valid" map is anchored at the window's first pixel) of both frames as
//                               bytes in LDS, then for each of the four planes R, G, B, Y: widens the plane to float64, runs the window down
//                               the columns (five moments: x, y, x^2, y^2, xy), runs it along the rows of those, forms the SSIM value of
//                               each map position and adds it up.  The squared differences of its own pixels are added as integers (R, G, B)
//                               and as float64 (Y).  Sums are reduced by wavefront shuffles, then across the four wavefronts through LDS, and
//                               leave as one 48-byte record per workgroup.
//   frame_metrics_reduce_kernel one workgroup per frame adds that frame's records in a fixed order.
// Everything is float64 or integer: sigma^2 = E[x^2] - mu^2 cancels at magnitude 65 025 against C2 = 58.5, which float32 cannot carry
// (a flat 200 / 201 pair is then wrong in the fifth decimal).  No atomics, no transcendental function: two runs give the same bits,
// and the logarithm of PSNR is the host's, on the exact sums.
#include "common.h"

namespace {

constexpr int TW = 32, TH = 16;    // tile of map positions / owned pixels per workgroup
constexpr int HALO = 10;           // 11 taps - 1
constexpr int SW = TW + HALO, SH = TH + HALO;
constexpr int NREC = 6;            // 8-byte words per record: SSE of RGB (integer), SSE of Y, SSIM sums of R, G, B, Y

struct FrameView {
  const unsigned char* p;
  long long sf, sc, sr, sp;  // element strides: frame, channel, row, pixel
};
struct Window {
  double w[11];
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void stage_bytes(unsigned char* dst, const FrameView& v, int f, int y0, int x0, int H, int W) {
  const unsigned char* base = v.p + f * v.sf;
  // consecutive lanes follow the layout's fastest axis: channels of a pixel for interleaved frames, pixels of a row for planar ones
  const bool ch_fast = v.sc < v.sp;
  for (int i = threadIdx.x; i < 3 * SH * SW; i += 256) {
    int c, r, x;
    if (ch_fast) {
      c = i % 3;
      x = (i / 3) % SW;
      r = i / (3 * SW);
    } else {
      x = i % SW;
      r = (i / SW) % SH;
      c = i / (SW * SH);
    }
    const int gy = y0 + r, gx = x0 + x;
    unsigned char val = 0;
    if (gy < H && gx < W) val = base[c * v.sc + gy * v.sr + gx * v.sp];
    dst[(c * SH + r) * SW + x] = val;
  }
}

// rgb2ycbcr(uint8)[..., 0] of scikit-image, not rounded (tools/test_reds4.py:208-209)
__device__ __forceinline__ double luma(const unsigned char* s, int i) {
  return 16.0 + (65.481 * (double)s[i] + 128.553 * (double)s[SH * SW + i] + 24.966 * (double)s[2 * SH * SW + i]) / 255.0;
}

__global__ __launch_bounds__(256) void frame_metrics_tile_kernel(FrameView A, FrameView B, int H, int W, Window win, double C1, double C2,
                                                                 double* __restrict__ ws) {
  __shared__ unsigned char sA[3 * SH * SW], sB[3 * SH * SW];
  __shared__ double pX[SH * SW], pY[SH * SW];
  __shared__ double V[5][TH][SW];
  __shared__ double red[4][NREC];

  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, f = blockIdx.z;
  const int own_r = min(TH, H - y0), own_c = min(TW, W - x0);                  // pixels this tile owns (>= 1)
  const int map_r = min(TH, H - HALO - y0), map_c = min(TW, W - HALO - x0);    // map positions it owns (may be <= 0)
  const int in_c = min(SW, W - x0);                                            // staged columns that exist

  stage_bytes(sA, A, f, y0, x0, H, W);
  stage_bytes(sB, B, f, y0, x0, H, W);
  __syncthreads();

  long long sse = 0;
  double sse_y = 0.0, ssim[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < TH * TW; i += 256) {
    const int r = i / TW, c = i % TW;
    if (r < own_r && c < own_c) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int d = (int)sA[(ch * SH + r) * SW + c] - (int)sB[(ch * SH + r) * SW + c];
        sse += d * d;
      }
    }
  }

#pragma unroll 1
  for (int plane = 0; plane < 4; ++plane) {
    // the plane of both frames as float64 (the previous plane's column pass is behind the barrier in front of its row pass)
    for (int i = tid; i < SH * SW; i += 256) {
      double a, b;
      if (plane < 3) {
        a = (double)sA[plane * SH * SW + i];
        b = (double)sB[plane * SH * SW + i];
      } else {
        a = luma(sA, i);
        b = luma(sB, i);
        const int r = i / SW, c = i % SW;
        if (r < own_r && c < own_c) sse_y += (a - b) * (a - b);
      }
      pX[i] = a;
      pY[i] = b;
    }
    __syncthreads();
    // window down the columns
    for (int i = tid; i < TH * SW; i += 256) {
      const int r = i / SW, c = i % SW;
      if (r < map_r && c < in_c) {
        double m1 = 0.0, m2 = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
          const double a = pX[(r + k) * SW + c], b = pY[(r + k) * SW + c];
          const double wa = win.w[k] * a, wb = win.w[k] * b;
          m1 += wa;
          m2 += wb;
          xx += wa * a;
          yy += wb * b;
          xy += wa * b;
        }
        V[0][r][c] = m1;
        V[1][r][c] = m2;
        V[2][r][c] = xx;
        V[3][r][c] = yy;
        V[4][r][c] = xy;
      }
    }
    __syncthreads();
    // window along the rows, then the map value (utils/metrics.py:59-69)
    for (int i = tid; i < TH * TW; i += 256) {
      const int r = i / TW, c = i % TW;
      if (r < map_r && c < map_c) {
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 11; ++k) {
#pragma unroll
          for (int q = 0; q < 5; ++q) m[q] += win.w[k] * V[q][r][c + k];
        }
        const double mu1_sq = m[0] * m[0], mu2_sq = m[1] * m[1], mu1_mu2 = m[0] * m[1];
        const double s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu1_mu2;
        ssim[plane] += ((2.0 * mu1_mu2 + C1) * (2.0 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
      }
    }
  }

  sse = wave_sum_i64(sse);
  sse_y = wave_sum_f64(sse_y);
#pragma unroll
  for (int q = 0; q < 4; ++q) ssim[q] = wave_sum_f64(ssim[q]);
  const int wave = tid >> 6;
  if ((tid & 63) == 0) {
    red[wave][0] = __longlong_as_double(sse);
    red[wave][1] = sse_y;
#pragma unroll
    for (int q = 0; q < 4; ++q) red[wave][2 + q] = ssim[q];
  }
  __syncthreads();
  if (tid < NREC) {
    const long long nblk = (long long)gridDim.x * gridDim.y;
    double* rec = ws + ((long long)f * nblk + (long long)blockIdx.y * gridDim.x + blockIdx.x) * NREC;
    if (tid == 0) {
      long long s = 0;
      for (int w = 0; w < 4; ++w) s += __double_as_longlong(red[w][0]);
      rec[0] = __longlong_as_double(s);
    } else {
      double s = 0.0;
      for (int w = 0; w < 4; ++w) s += red[w][tid];
      rec[tid] = s;
    }
  }
}

__global__ __launch_bounds__(256) void frame_metrics_reduce_kernel(const double* __restrict__ ws, long long nblk, long long* __restrict__ sse_rgb,
                                                                   double* __restrict__ sums) {
  __shared__ double part[256][NREC];
  const int tid = threadIdx.x, f = blockIdx.x;
  const double* rec = ws + (long long)f * nblk * NREC;
  long long sse = 0;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long i = tid; i < nblk; i += 256) {
    sse += __double_as_longlong(rec[i * NREC]);
#pragma unroll
    for (int q = 0; q < 5; ++q) s[q] += rec[i * NREC + 1 + q];
  }
  part[tid][0] = __longlong_as_double(sse);
#pragma unroll
  for (int q = 0; q < 5; ++q) part[tid][1 + q] = s[q];
  __syncthreads();
  for (int step = 128; step > 0; step >>= 1) {
    if (tid < step) {
      part[tid][0] = __longlong_as_double(__double_as_longlong(part[tid][0]) + __double_as_longlong(part[tid + step][0]));
#pragma unroll
      for (int q = 1; q < NREC; ++q) part[tid][q] += part[tid + step][q];
    }
    __syncthreads();
  }
  if (tid == 0) sse_rgb[f] = __double_as_longlong(part[0][0]);
  if (tid >= 1 && tid < NREC) sums[(long long)f * 5 + tid - 1] = part[0][tid];
}

bool metrics_shape_ok(int T, int H, int W) { return T >= 1 && T <= 65535 && H >= 11 && W >= 11 && H <= (1 << 16) && W <= (1 << 16); }

}  // namespace

extern "C" int64_t vmg_frame_metrics_ws_bytes(int T, int H, int W) {
  if (!metrics_shape_ok(T, H, W)) return 0;
  return (int64_t)T * cdiv(W, TW) * cdiv(H, TH) * NREC * (int64_t)sizeof(double);
}

extern "C" int vmg_frame_metrics(const unsigned char* a, const int64_t* a_strides, const unsigned char* b, const int64_t* b_strides, int T, int H,
                                 int W, const double* window, void* ws, int64_t ws_bytes, int64_t* sse_rgb, double* sums, void* stream) {
  VMG_CHECK(T >= 1 && T <= 65535, "frame_metrics: 1 to 65535 frames per call, got %d", T);
  VMG_CHECK(H >= 11 && W >= 11, "frame_metrics: a %d x %d frame is smaller than the 11 x 11 SSIM window (its map is empty)", H, W);
  VMG_CHECK(H <= (1 << 16) && W <= (1 << 16), "frame_metrics: frame too large");
  VMG_CHECK(a && b && a_strides && b_strides && window && ws && sse_rgb && sums, "frame_metrics: null argument");
  VMG_CHECK(ws_bytes >= vmg_frame_metrics_ws_bytes(T, H, W), "frame_metrics: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
            (long long)vmg_frame_metrics_ws_bytes(T, H, W));
  VMG_CHECK(((uintptr_t)ws & 7) == 0 && ((uintptr_t)sse_rgb & 7) == 0 && ((uintptr_t)sums & 7) == 0, "frame_metrics: workspace and outputs must be 8-byte aligned");
  for (int i = 0; i < 4; ++i) VMG_CHECK(a_strides[i] >= 0 && b_strides[i] >= 0, "frame_metrics: negative stride");
  FrameView A{a, a_strides[0], a_strides[1], a_strides[2], a_strides[3]};
  FrameView B{b, b_strides[0], b_strides[1], b_strides[2], b_strides[3]};
  Window win;
  for (int k = 0; k < 11; ++k) win.w[k] = window[k];
  const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);  // utils/metrics.py:51-52
  const dim3 grid(cdiv(W, TW), cdiv(H, TH), T);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(frame_metrics_tile_kernel, grid, dim3(256), 0, st, A, B, H, W, win, C1, C2, (double*)ws);
  VMG_LAUNCH_CHECK();
  hipLaunchKernelGGL(frame_metrics_reduce_kernel, dim3(T), dim3(256), 0, st, (const double*)ws, (long long)grid.x * grid.y, (long long*)sse_rgb, sums);
  VMG_LAUNCH_CHECK();
  return 0;
}
