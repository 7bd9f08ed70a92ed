// Weight / bias gradient of the stride-1 "same" convolution (KS = 3 or 1), channels-last, gfx950.
//
//   dW[o][i][tap] += scale * sum_pixels dY[p][o] * X[p + tap][i]          (fp32, OIHW, atomically accumulated)
//
// GEMM view: M = output channels, N = (tap, input channel), K = pixels.  Both operands are stored pixel-major
// (channels-last), but the MFMA wants 8 consecutive K (= pixels) per lane, i.e. the TRANSPOSE of what is in
// memory.  gfx950's ds_read_b64_tr_b16 does that transpose on the LDS read path for 16-bit data: tiles are
// staged in LDS exactly as they lie in HBM ([pixel][channel], 16-byte vector copies) and each operand fragment
// is two transposed reads.  The tap shift is a row (pixel) offset of the transposed read, so one staged X tile
// with a 1-pixel halo serves all 9 taps.  fp32 uses v_mfma_f32_16x16x4_f32, whose operands are single
// elements (plain ds_read_b32).
//
// Work split: blockIdx.x = block of CT*16 output channels, blockIdx.y = block of IT*16 input channels,
// blockIdx.z = K split.  A K unit is 32 consecutive pixels of one image row.  Each of the 4 waves walks its own
// units through a wave-private LDS tile (no workgroup barriers in the main loop; next unit's global loads are in
// flight while the current one is multiplied).  At the end the 4 waves' accumulators are summed with LDS float
// atomics into a [co][ci][tap] image = the OIHW order, and written out with coalesced global float atomics.
#include <stdlib.h>
#include <algorithm>
#include <type_traits>

#include "common.h"

namespace {

constexpr int WG_MAX_PAIRS = 16;  // (x, dy) pairs summed by one launch (uses of a shared weight)
// Which MFMA kernel this file launched last (vmg_conv_wgrad_last_kernel, include/vmg_hip.h VMG_WGRAD_*): written on the host next to every
// launch, so that a test can tell which kernel the dispatch below picked for its shape.  kind << 24 | a << 16 | b << 8 | c.
int g_last_kernel = 0;
constexpr int last_kernel_id(int kind, int a = 0, int b = 0, int c = 0) { return kind << 24 | a << 16 | b << 8 | c; }
__device__ __attribute__((aligned(256))) unsigned int g_zero_buf[64];  // 256 zero bytes: load / DMA source for out-of-image lanes

// LDS-DMA (1 KiB per wave: 16 bytes per lane from a per-lane global address into a lane-linear LDS block) as an asm statement: when a
// wave issues the BUILTIN, hipcc treats every later ds_read of that wave as possibly aliasing the copy and puts s_waitcnt vmcnt(0) in
// front of it -- the copies in flight (the whole prefetch ring) are then waited for before every fragment read, and copies and MFMAs
// run one after the other (measured on the 3x3 kernel: copies alone 39 us, MFMAs + reads 52 us, together 89 us).  Hidden in asm the
// copies are counted by hand (the s_waitcnt vmcnt(N) before the barriers); M0 is saved and restored inside the statement.
__device__ __forceinline__ void glds16_hidden(const char* gsrc, char* lds_dst) {
  unsigned keep;
  const unsigned ldst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)LDS_PTR(lds_dst));  // (wave-uniform by construction)
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(ldst) : "memory");
}

// The gx * gy workgroups of one K slab stream the SAME dY / X lines.  The hardware hands workgroup L of a 1-D grid to XCD L % 8 (each XCD
// has its own L2), so the logical index is permuted: the blocks of a slab are consecutive on ONE XCD, run at the same time and
// share the lines through that L2 instead of fetching them gx * gy times from HBM.
struct SlabBlock { int x, y, z; };
__device__ __forceinline__ SlabBlock xcd_slab_block(int gx, int gy, int S) {
  const int T = gx * gy * S, L = blockIdx.x;
  const int xcd = L & 7, j = L >> 3, rem = T & 7;
  const int w = xcd * (T >> 3) + (xcd < rem ? xcd : rem) + j;
  SlabBlock b;
  b.x = w % gx;
  const int t = w / gx;
  b.y = t % gy;
  b.z = t / gy;
  return b;
}

struct WgradK {
  const char* x[WG_MAX_PAIRS];
  const char* dy[WG_MAX_PAIRS];
  int npairs;
  long long Upair;  // K units per pair
  long long x_ps;
  int Cin;
  long long dy_ps;
  int Cout;
  float* dW;
  int I_total, o0, i0;
  float* db;
  float scale;
  int N, H, W, SEG;
  int HB;  // row blocks per image (KS > 1: a K unit is UR rows x 32 pixels)
  long long M, U;
  int S;
  int vec_x, vec_dy;  // 16-byte vector loads are legal for the operand (pixel stride, channel count and base address are vector multiples)
  float* slab;  // non-null: every workgroup STORES its partial tile to slab[z][y][x][tile] (a reduce kernel sums the K splits in a fixed
                // order) instead of adding it to dW with float atomics -- with few (co, ci) tiles and many K splits the atomics all hit the
                // same few addresses and serialise (7x7: 131 us of a 140 us launch)
};

// UR: image rows per K unit (a unit = UR rows x 32 pixels).  The X tile with its halo is (UR + KS - 1) x (32 + KS - 1) pixels: for 7x7
// one row per unit re-loads 7 rows of halo per 32 pixels; four rows per unit cut the X traffic per pixel 2.8-fold.
template <typename T, int KS, int CT, int IT, int UR = 1>
struct WgradCfg {
  static constexpr int ES = ElemTraits<T>::ES;
  static constexpr int KK = KS * KS;
  static constexpr int XR = KS + UR - 1, XW = 32 + KS - 1;
  static constexpr int UP = UR * 32;  // pixels per unit
  static constexpr int DYC = CT * 16, XC = IT * 16;
  static constexpr int DY_RS = DYC * ES + 16, X_RS = XC * ES + 16;  // LDS row (= pixel) strides in bytes
  static constexpr int DY_BYTES = UP * DY_RS, X_BYTES = XR * XW * X_RS;
  static constexpr int WAVE_BYTES = (DY_BYTES + X_BYTES + 15) & ~15;
  static constexpr int RED_RS = XC * KK + 2;  // floats per output-channel row of the reduction image
  static constexpr int RED_BYTES = (DYC * RED_RS + DYC) * 4;
  // the reduction image takes over the waves' tiles once the main loop is done (behind a barrier)
  static constexpr int LDS_BYTES = 4 * WAVE_BYTES > RED_BYTES ? 4 * WAVE_BYTES : RED_BYTES;
  static constexpr int VPL = 16 / ES;                        // elements per 16-byte vector
  static constexpr int DY_VPP = DYC / VPL, X_VPP = XC / VPL;  // vectors per pixel
  static constexpr int DY_NV = (UP * DY_VPP + 63) / 64, X_NV = (XR * XW * X_VPP + 63) / 64;  // vectors per lane
};

__device__ __forceinline__ bf16x8 tr_frag(const char* tile, int rs, int k0, int c0, int lane) {
  // operand fragment of v_mfma_f32_16x16x32_bf16 from a [pixel][channel] LDS tile: lane l gets channel c0+(l&15),
  // pixels k0 + 8*(l>>4) + 0..7.  Two transposed 4x16 block reads (cdna guide T10): lane i = 4q+p of a 16-lane
  // group supplies the address of block row q, columns 4p..4p+3.
  const int i = lane & 15, g = lane >> 4;
  const char* p0 = tile + (k0 + 8 * g + (i >> 2)) * rs + (c0 + 4 * (i & 3)) * 2;
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p0));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p0 + 4 * rs));
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

template <typename T, int KS, int CT, int IT, int UR = 1>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const WgradK a) {
  using C = WgradCfg<T, KS, CT, IT, UR>;
  constexpr int ES = C::ES, KK = C::KK;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  char* dyt = smem + wave * C::WAVE_BYTES;
  char* xt = dyt + C::DY_BYTES;
  float* red = reinterpret_cast<float*>(smem);  // (valid behind the barrier that follows the main loop)
  float* redb = red + C::DYC * C::RED_RS;

  const int ob = blockIdx.x * C::DYC, ib = blockIdx.y * C::XC;  // channel offsets of this block
  const long long u_lo = a.U * blockIdx.z / a.S, u_hi = a.U * (blockIdx.z + 1) / a.S;
  const bool do_bias = (a.db != nullptr) && (blockIdx.y == 0);

  f32x4 acc[CT][KK][IT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int t = 0; t < KK; ++t)
#pragma unroll
      for (int it = 0; it < IT; ++it) acc[ct][t][it] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;

  uint4 rdy[C::DY_NV], rx[C::X_NV];
  const char* zsrc = reinterpret_cast<const char*>(g_zero_buf);

  auto load_unit = [&](long long ug) {
    // which (x, dy) pair, then pixel coordinates of the unit inside it
    const int pair = (int)(ug / a.Upair);
    const long long u = ug - (long long)pair * a.Upair;
    const char* xbase = a.x[pair];
    const char* dybase = a.dy[pair];
    int n = 0, y = 0, x0 = 0;
    long long m0 = 0;
    if (KS > 1) {
      const int seg = (int)(u % a.SEG);
      const long long r = u / a.SEG;
      y = (int)(r % a.HB) * UR;
      n = (int)(r / a.HB);
      x0 = seg * 32;
    } else {
      m0 = u * 32;
    }
    // Every load is UNCONDITIONAL: a lane outside the image (or past the channels) reads the zero buffer instead.  Loads behind a
    // per-lane branch are each followed by an s_waitcnt vmcnt(0) -- ten serialised memory latencies per unit, which made even the
    // 2 x 2-pixel SPyNet level cost 100 us.
    auto dy_src = [&](int k, bool& ok, int& c) -> const char* {
      const int idx = lane + 64 * k;
      const int p = idx / C::DY_VPP, v = idx - p * C::DY_VPP;
      c = ob + v * C::VPL;
      ok = (idx < C::UP * C::DY_VPP);
      long long pix;
      if (KS > 1) {
        const int rr = p >> 5, col = p & 31;
        ok = ok && (x0 + col < a.W) && (y + rr < a.H);
        pix = ((long long)n * a.H + y + rr) * a.W + x0 + col;
      } else { ok = ok && (m0 + p < a.M); pix = m0 + p; }
      return dybase + (pix * a.dy_ps + c) * ES;
    };
    auto x_src = [&](int k, bool& ok, int& c) -> const char* {
      const int idx = lane + 64 * k;
      const int p = idx / C::X_VPP, v = idx - p * C::X_VPP;
      c = ib + v * C::VPL;
      ok = (idx < C::XR * C::XW * C::X_VPP);
      long long pix;
      if (KS > 1) {
        const int r = p / C::XW, col = p - r * C::XW;
        const int yy = y + r - KS / 2, xx = x0 + col - KS / 2;
        ok = ok && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
        pix = ((long long)n * a.H + yy) * a.W + xx;
      } else {
        ok = ok && (m0 + p < a.M);
        pix = m0 + p;
      }
      return xbase + (pix * a.x_ps + c) * ES;
    };
    if (a.vec_dy) {
#pragma unroll
      for (int k = 0; k < C::DY_NV; ++k) {
        bool ok; int c;
        const char* src = dy_src(k, ok, c);
        rdy[k] = *reinterpret_cast<const uint4*>((ok && c < a.Cout) ? src : zsrc);  // (a vector that starts inside the channels ends inside the pixel stride: channels past Cout are computed and dropped)
      }
    } else {
#pragma unroll
      for (int k = 0; k < C::DY_NV; ++k) {
        bool ok; int c;
        const char* src = dy_src(k, ok, c);
        T tmp[C::VPL];
#pragma unroll
        for (int e = 0; e < C::VPL; ++e) tmp[e] = *reinterpret_cast<const T*>((ok && c + e < a.Cout) ? src + e * ES : zsrc);
        rdy[k] = *reinterpret_cast<const uint4*>(tmp);
      }
    }
    if (a.vec_x) {
#pragma unroll
      for (int k = 0; k < C::X_NV; ++k) {
        bool ok; int c;
        const char* src = x_src(k, ok, c);
        rx[k] = *reinterpret_cast<const uint4*>((ok && c < a.Cin) ? src : zsrc);
      }
    } else {
#pragma unroll
      for (int k = 0; k < C::X_NV; ++k) {
        bool ok; int c;
        const char* src = x_src(k, ok, c);
        T tmp[C::VPL];
#pragma unroll
        for (int e = 0; e < C::VPL; ++e) tmp[e] = *reinterpret_cast<const T*>((ok && c + e < a.Cin) ? src + e * ES : zsrc);
        rx[k] = *reinterpret_cast<const uint4*>(tmp);
      }
    }
  };

  auto store_unit = [&]() {
#pragma unroll
    for (int k = 0; k < C::DY_NV; ++k) {
      const int idx = lane + 64 * k;
      const int p = idx / C::DY_VPP, v = idx - p * C::DY_VPP;
      if (idx < C::UP * C::DY_VPP) *reinterpret_cast<uint4*>(dyt + p * C::DY_RS + v * 16) = rdy[k];
    }
#pragma unroll
    for (int k = 0; k < C::X_NV; ++k) {
      const int idx = lane + 64 * k;
      const int p = idx / C::X_VPP, v = idx - p * C::X_VPP;
      if (idx < C::XR * C::XW * C::X_VPP) *reinterpret_cast<uint4*>(xt + p * C::X_RS + v * 16) = rx[k];
    }
  };

  long long u = u_lo + wave;
  if (u < u_hi) load_unit(u);
  while (u < u_hi) {
    store_unit();
    const long long un = u + 4;
    if (un < u_hi) load_unit(un);
    // wave-private tile: program order + the compiler's lgkmcnt waits are the only synchronisation needed
#pragma unroll
    for (int rr = 0; rr < UR; ++rr) {
      if constexpr (ES == 2) {
        bf16x8 af[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) af[ct] = tr_frag(dyt, C::DY_RS, rr * 32, ct * 16, lane);
#pragma unroll
        for (int t = 0; t < KK; ++t) {
          const int ky = t / KS, kx = t % KS;
#pragma unroll
          for (int it = 0; it < IT; ++it) {
            const bf16x8 bfg = tr_frag(xt + (rr + ky) * C::XW * C::X_RS, C::X_RS, kx, it * 16, lane);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
              acc[ct][t][it] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ct], bfg, acc[ct][t][it], 0, 0, 0);
          }
        }
      } else {
        const int l15 = lane & 15, g = lane >> 4;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float af[CT];
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) af[ct] = *reinterpret_cast<const float*>(dyt + (rr * 32 + 4 * j + g) * C::DY_RS + (ct * 16 + l15) * 4);
#pragma unroll
          for (int t = 0; t < KK; ++t) {
            const int ky = t / KS, kx = t % KS;
#pragma unroll
            for (int it = 0; it < IT; ++it) {
              const float bv = *reinterpret_cast<const float*>(xt + ((rr + ky) * C::XW + 4 * j + g + kx) * C::X_RS + (it * 16 + l15) * 4);
#pragma unroll
              for (int ct = 0; ct < CT; ++ct)
                acc[ct][t][it] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[ct], bv, acc[ct][t][it], 0, 0, 0);
            }
          }
        }
      }
    }
    if (do_bias && lane < C::DYC) {
      float s = 0.f;
#pragma unroll 8
      for (int p = 0; p < C::UP; ++p) s += to_f32(*reinterpret_cast<const T*>(dyt + p * C::DY_RS + lane * ES));
      bsum += s;
    }
    u = un;
  }

  // ---- cross-wave reduction in LDS, laid out [co][ci][tap] = OIHW order of this block
  __syncthreads();  // every wave is done with its tiles: the reduction image reuses that memory
  for (int i = tid; i < C::DYC * C::RED_RS + C::DYC; i += 256) red[i] = 0.f;
  __syncthreads();
  {
    const int l15 = lane & 15, g = lane >> 4;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int t = 0; t < KK; ++t)
#pragma unroll
        for (int it = 0; it < IT; ++it)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            atomicAdd(&red[(ct * 16 + 4 * g + r) * C::RED_RS + (it * 16 + l15) * KK + t], acc[ct][t][it][r]);
    if (do_bias && lane < C::DYC) atomicAdd(&redb[lane], bsum);
  }
  __syncthreads();
  constexpr int ROW = C::XC * KK;
  if (a.slab) {
    constexpr int TILE = C::DYC * ROW + C::DYC;  // floats per workgroup: the tile, then the bias sums
    float* dst = a.slab + (((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * TILE;
    for (int i = tid; i < C::DYC * ROW; i += 256) {
      const int co = i / ROW, rem = i - co * ROW;
      dst[i] = red[co * C::RED_RS + rem];
    }
    if (tid < C::DYC) dst[C::DYC * ROW + tid] = do_bias ? redb[tid] : 0.f;
    return;
  }
  for (int i = tid; i < C::DYC * ROW; i += 256) {
    const int co = i / ROW, rem = i - co * ROW;
    const int ci = rem / KK;
    if (ob + co < a.Cout && ib + ci < a.Cin)
      atomicAdd(&a.dW[((long long)(a.o0 + ob + co) * a.I_total + (a.i0 + ib)) * KK + rem], red[co * C::RED_RS + rem] * a.scale);
  }
  if (do_bias && tid < C::DYC && ob + tid < a.Cout) atomicAdd(&a.db[a.o0 + ob + tid], redb[tid] * a.scale);
}

// sums the K splits of the slab form in a fixed order and adds the result to dW / db (one thread per element: no atomics)
__global__ void wgrad_slab_reduce_kernel(const float* __restrict__ slab, int S, int gx, int gy, int DYC, int XC, int KK, int Cout, int Cin,
                                         float* __restrict__ dW, int I_total, int o0, int i0, float* __restrict__ db, float scale) {
  const int ROW = XC * KK, TILE = DYC * ROW + DYC;
  const long long total = (long long)gx * gy * TILE;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int e = (int)(i % TILE);
    const int bxy = (int)(i / TILE);
    const int bx = bxy % gx, by = bxy / gx;
    float s = 0.f;
    for (int z = 0; z < S; ++z) s += slab[((size_t)z * gy * gx + bxy) * TILE + e];
    if (e < DYC * ROW) {
      const int co = e / ROW, rem = e - co * ROW, ci = rem / KK;
      if (bx * DYC + co < Cout && by * XC + ci < Cin)
        dW[((long long)(o0 + bx * DYC + co) * I_total + (i0 + by * XC)) * KK + rem] += s * scale;
    } else if (db && by == 0) {
      const int co = e - DYC * ROW;
      if (bx * DYC + co < Cout) db[o0 + bx * DYC + co] += s * scale;
    }
  }
}

}  // namespace

// =====================================================================================================
// Large-tile kernels (bf16): shared LDS tiles, slab reduction.
//
// The v1 kernel above gives every workgroup a 48 x 16 x 9 output tile, so dY is re-read 9x and X 3x from L2/HBM (1.2 GB
// for the batched gradient of one recurrent conv) and the float-atomic epilogue scales with the number of K splits.
// Here a workgroup owns ALL 144 output channels x 48 input channels x 9 taps (3x3) or 144 x 144 (1x1).  Per 32-pixel K
// unit the dY tile [32][144] and the X tile ([3][34][48] with its halo, or [32][144]) are filled by LDS-DMA
// (global_load_lds, per-lane source, lane-linear destination; out-of-image lanes read a zero buffer, so every wave issues
// the same number of DMA instructions per unit and the wait can be COUNTED) and read transposed.  Partial results go to
// per-slab workspaces in the accumulator's native layout with coalesced float4 stores; a second kernel sums the slabs in
// a fixed order (bitwise reproducible, unlike atomics) and adds them into the OIHW gradient.  The bias gradient is one
// more MFMA per co tile against a ones operand.
// =====================================================================================================
namespace {


constexpr int W3_MAX_PROBS = 8;  // weight-gradient problems of one shape served by one launch (vmg_conv_wgrad3_multi)
struct Wgrad2K {
  const char* x[W3_MAX_PROBS * WG_MAX_PAIRS];   // [problem][pair]
  const char* dy[W3_MAX_PROBS * WG_MAX_PAIRS];
  int npairs, nprob;
  long long Upair, U;  // K units per pair / per problem
  long long x_ps, dy_ps;
  int Cin, Cout;
  float* slab;       // [problem][S][ciblk][coblk][8 waves][36 tiles][64][4]
  int N, H, W, SEG, S;
  int has_bias;
  int gx, gy;        // co / ci blocks (the grid is 1-D: gx * gy * S * nprob workgroups, see xcd_slab_block)
  int dbg;           // diagnostics build only (env VMG_WGRAD_DBG): 1 no copies after the prologue, 2 no MFMAs, 4 no fragment reads
};
struct Wgrad3Out {   // per problem: where the reduce kernel adds the sums
  float* dW[W3_MAX_PROBS];
  float* db[W3_MAX_PROBS];
  float scale[W3_MAX_PROBS];
};

constexpr int W2_WAVES = 9, W2_THREADS = 576;  // the 1x1 kernel's workgroup
constexpr int W2_DYC = 144, W2_XC = 48, W2_XR = 3, W2_XW = 34;
constexpr int W2_XVEC = W2_XR * W2_XW * (W2_XC / 8);        // 612 vectors in the X tile

// Sum of element i over the S slabs, in a FIXED order (deterministic): the block's 4 waves each take the slabs
// s = w, w+4, ... (coalesced 256-byte rows, 4 loads in flight), the 4 partial sums are combined through LDS as
// ((p0 + p1) + (p2 + p3)).  Call with blockDim = 256; lane l of every wave works on element i0 + l; returns the sum on
// wave 0 (other waves get an unspecified value).
__device__ __forceinline__ float slab_sum_4waves(const float* __restrict__ slab, long long per_s, int S, long long i, bool valid, float* red) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (valid) {
    int s = w;
    for (; s + 12 < S; s += 16) {
      a0 += slab[(long long)s * per_s + i];
      a1 += slab[(long long)(s + 4) * per_s + i];
      a2 += slab[(long long)(s + 8) * per_s + i];
      a3 += slab[(long long)(s + 12) * per_s + i];
    }
    for (; s < S; s += 4) a0 += slab[(long long)s * per_s + i];
  }
  red[w * 64 + l] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  const float r = (red[l] + red[64 + l]) + (red[128 + l] + red[192 + l]);
  __syncthreads();
  return r;
}

// =====================================================================================================
// 3x3: the tile (144 co x 48 ci x 9 taps per workgroup) on EIGHT waves, two per SIMD.
// (A nine-wave 3 x 3 layout of the same tile put three waves on one SIMD -- its MFMA share bounded every unit -- and left
// 170 registers per wave, too few for a second fragment set: LDS reads and MFMAs ran one after the other; 161 us vs 124 us
// for the 7-use gradient of a recurrent conv.)  Wave (h, q) owns co tiles
// 5h..5h+4 (h = 1: four real tiles) x fragment columns 7q..7q+6 of the 27 (ci tile, tap) columns = 35 accumulator
// tiles; with 256 registers the X fragment of the NEXT unit is read into the registers of the fragment just consumed,
// so LDS reads run under the MFMAs.  Per unit the [dY tile | X tile] pair is one linear list of 1188 16-byte vectors
// copied by LDS-DMA, three 1-KiB instructions per wave (lanes past the list or outside the image read a zero buffer):
// the wait is COUNTED.  Six LDS unit slots, one barrier per two units; slab partials + ordered reduction.
// =====================================================================================================
constexpr int W3_WAVES = 8, W3_THREADS = 512, W3_SLOTS = 3;
constexpr int W3_DYV = 576, W3_VECS = 576 + W2_XVEC;            // 1188 vectors per unit
constexpr int W3_BUF = W3_SLOTS * W3_WAVES * 1024;               // 24576 B per buffer (every wave issues 3 full instructions)
constexpr int W3_TILES = 36;                                     // 35 accumulator tiles + 1 bias tile per wave
constexpr long long W3_WG_FLOATS = (long long)W3_WAVES * W3_TILES * 256;

__device__ __forceinline__ bf16x8 tr_read(const char* p0, int rs) {
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p0));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p0 + 4 * rs));
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

typedef __attribute__((ext_vector_type(4))) unsigned int w3_u32x4;
// LDS-DMA through a buffer resource: 16 bytes per lane from (descriptor base + SGPR offset + per-lane 32-bit offset) into the lane-linear 1 KiB
// block at lds_dst; a lane whose offset is >= num_records (2^31 here) gets zeros.  Hidden from hipcc's wait bookkeeping like glds16_hidden; the
// s_nop covers the M0 write and SGPRs the compiler's SALU may have written just before the statement (descriptor, offset).
__device__ __forceinline__ void bufdma16_hidden(unsigned voff, w3_u32x4 rsrc, unsigned soff, char* lds_dst) {
  unsigned keep;
  const unsigned ldst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)LDS_PTR(lds_dst));
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(soff), "s"(ldst) : "memory");
}
__device__ __forceinline__ w3_u32x4 w3_rsrc(const char* base) {  // raw buffer (stride 0) of 2^31 bytes at `base` (wave-uniform)
  const unsigned long long p = (unsigned long long)(uintptr_t)base;
  w3_u32x4 r;
  r[0] = __builtin_amdgcn_readfirstlane((unsigned)p);
  r[1] = __builtin_amdgcn_readfirstlane((unsigned)(p >> 32)) & 0xFFFFu;
  r[2] = 0x80000000u;
  r[3] = 0x00020000u;
  return r;
}

__global__ __launch_bounds__(W3_THREADS) void conv_wgrad3_kernel(const Wgrad2K a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = wave >> 2, q = wave & 3;
  SlabBlock blk = xcd_slab_block(a.gx, a.gy, a.S * a.nprob);
  const int prob = blk.z / a.S;  // several problems of one shape share the launch: fewer, longer K slabs per problem at a full chip
  const int zz = blk.z;          // slab index over all problems (the slab workspace is [problem][S]...)
  blk.z -= prob * a.S;
  const char* const* xs = a.x + prob * WG_MAX_PAIRS;
  const char* const* dys = a.dy + prob * WG_MAX_PAIRS;
  const int ob = blk.x * W2_DYC, ib = blk.y * W2_XC;
  const long long u_lo = a.U * blk.z / a.S, u_hi = a.U * (blk.z + 1) / a.S;
  const char* zsrc = reinterpret_cast<const char*>(g_zero_buf);

  f32x4 acc[5][7];
#pragma unroll
  for (int c = 0; c < 5; ++c)
#pragma unroll
    for (int j = 0; j < 7; ++j) acc[c][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 accb[5];
#pragma unroll
  for (int c = 0; c < 5; ++c) accb[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16 one = (bf16)1.0f;
  const bf16x8 ones = {one, one, one, one, one, one, one, one};

  // ---- copy instructions.  The kernel is bound by INSTRUCTION ISSUE, not by memory (with every copy an L2 hit it runs at the same
  // speed) nor by the matrix pipe: per 32-pixel unit a wave has 35 MFMAs (560 cycles) and, in the first version, ~450 other instructions
  // (per-lane 64-bit address arithmetic of the copies, 64-bit loop counters, slot rotation, fragment double buffers): 0.44 us of loop
  // skeleton + 0.57 us of copy issue + 0.5 us of MFMAs per unit.  Hence: a lane keeps a 64-bit POINTER per copy instruction and adds a
  // wave-uniform delta per unit; the loop is unrolled over the six LDS slots (static slot addresses, static barrier parity, 32-bit
  // counters); one fragment set, re-read behind the last MFMA that uses it.
  // Lane constants of the three copy instructions: vector L of the [dY | X] list.  Chunk sl * 8 + wave < 9 is a dY chunk, the rest X
  // (wave-uniform); abk = a | b << 8 | kind << 16, kind 0 dY (a = pixel), 1 X (a = row, b = column), 2 padding (reads the zero buffer).
  int s_abk[W3_SLOTS];
  const char* s_ptr[W3_SLOTS];  // source of the NEXT unit to be issued
  const int nun = (int)(u_hi - u_lo);
  int ipair = (int)(u_lo / a.Upair), iseg, iy, in_;
  {
    const long long uu = u_lo - (long long)ipair * a.Upair;
    iseg = (int)(uu % a.SEG);
    const long long r = uu / a.SEG;
    iy = (int)(r % a.H);
    in_ = (int)(r / a.H);
  }
  {
    const long long row0 = ((long long)in_ * a.H + iy) * a.W + iseg * 32;
#pragma unroll
    for (int sl = 0; sl < W3_SLOTS; ++sl) {
      const int L = (sl * W3_WAVES + wave) * 64 + lane;
      if (L < W3_DYV) {
        const int pp = L / 18, v = L - pp * 18;
        s_abk[sl] = pp | (((ob + v * 8 + 8 <= a.Cout) ? 0 : 2) << 16);
        s_ptr[sl] = dys[ipair] + ((row0 + pp) * a.dy_ps + ob + v * 8) * 2;
      } else if (L < W3_VECS) {
        const int vec = L - W3_DYV, pp = vec / 6, v = vec - pp * 6;
        const int rr = pp / W2_XW, col = pp - rr * W2_XW;
        s_abk[sl] = rr | (col << 8) | (((ib + v * 8 + 8 <= a.Cin) ? 1 : 2) << 16);
        s_ptr[sl] = xs[ipair] + ((row0 + (long long)(rr - 1) * a.W + (col - 1)) * a.x_ps + ib + v * 8) * 2;
      } else {
        s_abk[sl] = 2 << 16;
        s_ptr[sl] = zsrc;
      }
    }
  }
  const long long pair_pix = (long long)a.N * a.H * a.W;
  const int row_adv = a.W - (a.SEG - 1) * 32;  // pixels from the last segment of a row to the start of the next row
  auto issue = [&](int buf) __attribute__((always_inline)) {
    const int x0 = iseg * 32;
    char* dst = smem + buf * W3_BUF;
#pragma unroll
    for (int sl = 0; sl < W3_SLOTS; ++sl) {
      const int abk = s_abk[sl], kind = abk >> 16, sa = abk & 255, sb = (abk >> 8) & 255;
      bool ok;
      if (sl * W3_WAVES + wave < W3_DYV / 64) ok = (kind == 0) & ((unsigned)(x0 + sa) < (unsigned)a.W);
      else ok = (kind == 1) & ((unsigned)(iy + sa - 1) < (unsigned)a.H) & ((unsigned)(x0 + sb - 1) < (unsigned)a.W);
      glds16_hidden(ok ? s_ptr[sl] : zsrc, dst + (sl * W3_WAVES + wave) * 1024);
    }
    // odometer + the wave-uniform pointer deltas to the next unit
    long long adv = 32;  // pixels
    long long rebase_dy = 0, rebase_x = 0;
    if (++iseg == a.SEG) {
      iseg = 0;
      adv = row_adv;
      if (++iy == a.H) {
        iy = 0;
        if (++in_ == a.N) {
          in_ = 0;
          if (ipair + 1 < a.npairs) {  // next (x, dy) pair: back to pixel 0 of other tensors
            rebase_dy = dys[ipair + 1] - dys[ipair] - pair_pix * a.dy_ps * 2;
            rebase_x = xs[ipair + 1] - xs[ipair] - pair_pix * a.x_ps * 2;
          }
          ++ipair;
        }
      }
    }
    const long long d_dy = adv * a.dy_ps * 2 + rebase_dy, d_x = adv * a.x_ps * 2 + rebase_x;
#pragma unroll
    for (int sl = 0; sl < W3_SLOTS; ++sl) s_ptr[sl] += (sl * W3_WAVES + wave < W3_DYV / 64) ? d_dy : d_x;
  };

  // ---- fragment addresses (within a buffer): dY rows are 288 B, X rows 96 B; lane i = 4qq+pp of a 16-lane group supplies
  // block row qq, columns 4pp..4pp+3 of a transposed 4x16 block read
  const int li = lane & 15, lg = lane >> 4;
  const int a_off = (8 * lg + (li >> 2)) * (W2_DYC * 2) + (h * 5 * 16 + 4 * (li & 3)) * 2;  // + c * 32 for co tile c of this wave
  int b_off[7];
#pragma unroll
  for (int jj = 0; jj < 7; ++jj) {
    const int col = min(q * 7 + jj, 26), itile = col / 9, tap = col - 9 * itile, ky = tap / 3, kx = tap - 3 * ky;
    b_off[jj] = W3_DYV * 16 + ky * W2_XW * (W2_XC * 2) + (kx + 8 * lg + (li >> 2)) * (W2_XC * 2) + (itile * 16 + 4 * (li & 3)) * 2;
  }

  // SIX unit slots, one barrier per TWO units.  Unit j lives in slot j % 6; iteration j multiplies unit j (fragments already in
  // registers) and reads unit j+1's fragments.  At the barrier of an even j every wave has (a) waited for its share of units
  // j+1 and j+2 (units j+3, j+4 stay in flight: the wait is counted) and (b) drained its reads of unit j; afterwards units
  // j+5 and j+6 are issued into the slots of units j-1 and j.
  for (int j = 0; j < 5; ++j)
    if (j < nun) issue(j);
  {
    const int later = nun > 3 ? (nun > 4 ? 2 : 1) : 0;  // units 3, 4 may stay in flight
    if (later == 2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if (later == 1) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  bf16x8 af[5], bfg[7];
  if (nun > 0) {
#pragma unroll
    for (int c = 0; c < 5; ++c) af[c] = tr_read(smem + a_off + c * 32, W2_DYC * 2);
#pragma unroll
    for (int jj = 0; jj < 7; ++jj) bfg[jj] = tr_read(smem + b_off[jj], W2_XC * 2);
  }
  const bool do_bias = a.has_bias && q == 0 && blk.y == 0;
  // one unit; SU = its slot (compile-time), j = its index.  Returns false when the slab is finished.
  auto unit = [&](int j, auto su_c) __attribute__((always_inline)) -> bool {
    constexpr int SU = decltype(su_c)::value, SN = (SU + 1) % 6, S5 = (SU + 5) % 6;
    constexpr bool SYNC = (SU & 1) == 0;  // slots alternate with the unit index: even units synchronise
    if (j >= nun) return false;
    if (SYNC) {
      const int later = (j + 3 < nun ? 1 : 0) + (j + 4 < nun ? 1 : 0);
      if (later == 2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      else if (later == 1) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's reads of unit j are complete
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
    const char* src = smem + ((j + 1 < nun) ? SN : SU) * W3_BUF;  // (last unit: re-read its own slot; the values are not used)
    // units j+5, j+6 -> the slots of units j-1 and j (free since this unit's barrier).  The two waves of a SIMD (h = 0, 1) are kept in
    // step by the barriers: h = 0 issues its copies BEFORE its MFMAs, h = 1 after them, so that one wave's address arithmetic runs
    // under the other wave's MFMAs instead of both leaving the matrix pipe idle at the same time.
    if (SYNC && h == 0) {
#ifdef VMG_DIAG
      if (!(a.dbg & 1))
#endif
      {
        if (j + 5 < nun) issue(S5);
        if (j + 6 < nun) issue(SU);
      }
    }
    if (do_bias) {
#pragma unroll
      for (int c = 0; c < 5; ++c) accb[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[c], ones, accb[c], 0, 0, 0);
    }
#pragma unroll
    for (int jj = 0; jj < 7; ++jj) {
#ifdef VMG_DIAG
      if (!(a.dbg & 2))
#endif
      {
#pragma unroll
        for (int c = 0; c < 5; ++c) acc[c][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[c], bfg[jj], acc[c][jj], 0, 0, 0);
      }
#ifdef VMG_DIAG
      if (!(a.dbg & 4))
#endif
      bfg[jj] = tr_read(src + b_off[jj], W2_XC * 2);
    }
#ifdef VMG_DIAG
    if (!(a.dbg & 4))
#endif
    {
#pragma unroll
      for (int c = 0; c < 5; ++c) af[c] = tr_read(src + a_off + c * 32, W2_DYC * 2);  // (behind the last MFMA that reads af[c])
    }
    if (SYNC && h == 1) {
#ifdef VMG_DIAG
      if (!(a.dbg & 1))
#endif
      {
        if (j + 5 < nun) issue(S5);
        if (j + 6 < nun) issue(SU);
      }
    }
    return true;
  };
  for (int base = 0; base < nun; base += 6) {
    if (!unit(base + 0, std::integral_constant<int, 0>{})) break;
    if (!unit(base + 1, std::integral_constant<int, 1>{})) break;
    if (!unit(base + 2, std::integral_constant<int, 2>{})) break;
    if (!unit(base + 3, std::integral_constant<int, 3>{})) break;
    if (!unit(base + 4, std::integral_constant<int, 4>{})) break;
    if (!unit(base + 5, std::integral_constant<int, 5>{})) break;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  // slab store: native accumulator layout, one float4 per lane per tile (fully coalesced)
  float* sl = a.slab + ((((long long)zz * a.gy + blk.y) * a.gx + blk.x) * W3_WAVES + wave) * (W3_TILES * 256);
#pragma unroll
  for (int c = 0; c < 5; ++c)
#pragma unroll
    for (int j = 0; j < 7; ++j) *reinterpret_cast<f32x4*>(sl + ((c * 7 + j) * 64 + lane) * 4) = acc[c][j];
  // bias tile: rows 4g..4g+3 of co tile c live in every column of D; column l15 < 5 of the slot carries co tile l15
  if (a.has_bias && q == 0 && blk.y == 0) {
    f32x4 pack = f32x4{0.f, 0.f, 0.f, 0.f};
    if (li < 5) pack = li == 0 ? accb[0] : (li == 1 ? accb[1] : (li == 2 ? accb[2] : (li == 3 ? accb[3] : accb[4])));
    *reinterpret_cast<f32x4*>(sl + (35 * 64 + lane) * 4) = pack;
  }
}

__global__ __launch_bounds__(W3_THREADS) void conv_wgrad3b_kernel(const Wgrad2K a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = wave >> 2, q = wave & 3;
  SlabBlock blk = xcd_slab_block(a.gx, a.gy, a.S * a.nprob);
  const int prob = blk.z / a.S;  // several problems of one shape share the launch: fewer, longer K slabs per problem at a full chip
  const int zz = blk.z;          // slab index over all problems (the slab workspace is [problem][S]...)
  blk.z -= prob * a.S;
  const char* const* xs = a.x + prob * WG_MAX_PAIRS;
  const char* const* dys = a.dy + prob * WG_MAX_PAIRS;
  const int ob = blk.x * W2_DYC, ib = blk.y * W2_XC;
  const long long u_lo = a.U * blk.z / a.S, u_hi = a.U * (blk.z + 1) / a.S;
  const char* zsrc = reinterpret_cast<const char*>(g_zero_buf);

  f32x4 acc[5][7];
#pragma unroll
  for (int c = 0; c < 5; ++c)
#pragma unroll
    for (int j = 0; j < 7; ++j) acc[c][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // The bias gradient rides on the tile's PADDING: wave q = 3 owns fragment columns 21..27 of 27, its seventh column is a duplicate that the
  // reduce kernel drops.  With a ones operand in its place that accumulator column is sum_p dY[p][co] -- no accumulators of its own (20
  // registers) and no extra MFMAs (round 2's kernel issues five more per unit on the q = 0 waves of the first ci block: 80 instead of 70 on SIMD 0).
  const bf16 one = (bf16)1.0f;
  const bf16x8 ones = {one, one, one, one, one, one, one, one};
  const bool bias_col = q == 3;

  // ---- copy instructions (round 4).  conv_wgrad3_kernel above keeps a 64-bit POINTER per lane and copy instruction, selects it against a
  // zero buffer with per-unit bounds tests and advances it by wave-uniform 64-bit deltas: ~60 instructions per unit and wave, issued as ONE
  // block before or after the unit's 35 MFMAs -- while a wave is in that block it feeds the matrix pipe nothing (the unit cost MFMAs + block:
  // 0.92 us where the MFMAs alone take 0.50).  Here the copies are BUFFER loads (`buffer_load_dwordx4 ... offen lds`): the tensor base sits in a
  // resource descriptor (SGPRs), the unit's first pixel in an SGPR byte offset that advances by precomputed 32-bit deltas, and a lane's offset
  // inside the [dY | X] list is a CONSTANT 32-bit register.  Which lanes fall outside the image depends on four wave-uniform facts only (first /
  // last row, first / last segment of a row): a lane carries its static flags, a unit its bits, and a flagged lane asks for offset 2^31 -- beyond
  // num_records, so the hardware writes zeros.  3 VALU per copy instruction instead of ~12, no zero buffer, no 64-bit lane arithmetic; and the
  // issue block of a unit shrinks from ~60 to ~25 instructions.
  unsigned voff[W3_SLOTS], flg[W3_SLOTS];
  const int nun = (int)(u_hi - u_lo);
  int ipair = (int)(u_lo / a.Upair), iseg, iy, in_;
  {
    const long long uu = u_lo - (long long)ipair * a.Upair;
    iseg = (int)(uu % a.SEG);
    const long long r = uu / a.SEG;
    iy = (int)(r % a.H);
    in_ = (int)(r / a.H);
  }
  const int wlast = a.W - (a.SEG - 1) * 32;  // pixels of a row's last segment
#pragma unroll
  for (int sl = 0; sl < W3_SLOTS; ++sl) {
    const int L = (sl * W3_WAVES + wave) * 64 + lane;
    if (L < W3_DYV) {
      const int pp = L / 18, v = L - pp * 18;
      voff[sl] = (unsigned)((pp * a.dy_ps + ob + v * 8) * 2);
      flg[sl] = 32u | (pp >= wlast ? 8u : 0u) | ((ob + v * 8 + 8 <= a.Cout) ? 0u : 16u);
    } else if (L < W3_VECS) {
      const int vec = L - W3_DYV, pp = vec / 6, v = vec - pp * 6;
      const int rr = pp / W2_XW, col = pp - rr * W2_XW;
      voff[sl] = (unsigned)(((long long)(rr * a.W + col) * a.x_ps + ib + v * 8) * 2);  // from the descriptor's base = one row and one pixel before the unit
      flg[sl] = 32u | (rr == 0 ? 1u : 0u) | (rr == 2 ? 2u : 0u) | (col == 0 ? 4u : 0u) | (col - 1 >= wlast ? 8u : 0u) | ((ib + v * 8 + 8 <= a.Cin) ? 0u : 16u);
    } else {
      voff[sl] = 0u;
      flg[sl] = 48u;
    }
  }
  const long long halo_x = (long long)(a.W + 1) * a.x_ps * 2;
  w3_u32x4 rs_dy = w3_rsrc(dys[ipair]), rs_x = w3_rsrc(xs[ipair] - halo_x);
  unsigned soff_dy, soff_x;
  {
    const long long row0 = ((long long)in_ * a.H + iy) * a.W + iseg * 32;
    soff_dy = (unsigned)(row0 * a.dy_ps * 2);
    soff_x = (unsigned)(row0 * a.x_ps * 2);
  }
  const unsigned a32_dy = (unsigned)(32 * a.dy_ps * 2), a32_x = (unsigned)(32 * a.x_ps * 2);
  const unsigned arow_dy = (unsigned)(wlast * a.dy_ps * 2), arow_x = (unsigned)(wlast * a.x_ps * 2);  // last segment of a row -> first pixel of the next row
  // Every copy instruction is UNCONDITIONAL: a unit past the end of the slab is issued as a DUMMY -- bit 32, which every lane carries, is set in
  // the unit's bits and all 64 lanes ask for offset 2^31 (zeros land in a free slot, no memory is touched).  Every wave then issues exactly six
  // copies per even iteration and every counted wait is vmcnt(6).
  unsigned ubits = 0;
  auto issue_slot = [&](int sl, int buf, unsigned dummy) __attribute__((always_inline)) {
    if (sl == 0) ubits = dummy | 16u | (iy == 0 ? 1u : 0u) | (iy == a.H - 1 ? 2u : 0u) | (iseg == 0 ? 4u : 0u) | (iseg == a.SEG - 1 ? 8u : 0u);
    const bool isdy = sl * W3_WAVES + wave < W3_DYV / 64;  // wave-uniform: chunks 0..8 of the list are dY
    const unsigned vo = (flg[sl] & ubits) ? 0x80000000u : voff[sl];
    bufdma16_hidden(vo, isdy ? rs_dy : rs_x, isdy ? soff_dy : soff_x, smem + buf * W3_BUF + (sl * W3_WAVES + wave) * 1024);
  };
  auto advance = [&]() __attribute__((always_inline)) {  // the odometer: to the unit after the one just issued
    unsigned d_dy = a32_dy, d_x = a32_x;
    if (++iseg == a.SEG) {
      iseg = 0;
      d_dy = arow_dy; d_x = arow_x;
      if (++iy == a.H) {
        iy = 0;
        if (++in_ == a.N) {
          in_ = 0;
          ++ipair;
          if (ipair < a.npairs) {  // next (x, dy) pair: other tensors, from their pixel 0
            rs_dy = w3_rsrc(dys[ipair]);
            rs_x = w3_rsrc(xs[ipair] - halo_x);
            soff_dy = 0u - d_dy;
            soff_x = 0u - d_x;
          }
        }
      }
    }
    soff_dy += d_dy;
    soff_x += d_x;
  };
  auto issue = [&](int buf, bool live) __attribute__((always_inline)) {
#pragma unroll
    for (int sl = 0; sl < W3_SLOTS; ++sl) issue_slot(sl, buf, live ? 0u : 32u);
    if (live) advance();
  };

  // ---- fragment addresses (within a buffer): dY rows are 288 B, X rows 96 B; lane i = 4qq+pp of a 16-lane group supplies
  // block row qq, columns 4pp..4pp+3 of a transposed 4x16 block read
  const int li = lane & 15, lg = lane >> 4;
  const int a_off = (8 * lg + (li >> 2)) * (W2_DYC * 2) + (h * 5 * 16 + 4 * (li & 3)) * 2;  // + c * 32 for co tile c of this wave
  int b_off[7];
#pragma unroll
  for (int jj = 0; jj < 7; ++jj) {
    const int col = min(q * 7 + jj, 26), itile = col / 9, tap = col - 9 * itile, ky = tap / 3, kx = tap - 3 * ky;
    b_off[jj] = W3_DYV * 16 + ky * W2_XW * (W2_XC * 2) + (kx + 8 * lg + (li >> 2)) * (W2_XC * 2) + (itile * 16 + 4 * (li & 3)) * 2;
  }

  // SIX unit slots, one barrier per TWO units.  Unit j lives in slot j % 6; iteration j multiplies unit j (fragments already in
  // registers) and reads unit j+1's fragments.  At the barrier of an even j every wave has (a) waited for its share of units
  // j+1 and j+2 (units j+3, j+4 stay in flight: the wait is counted) and (b) drained its reads of unit j; afterwards units
  // j+5 and j+6 are issued into the slots of units j-1 and j.
  for (int j = 0; j < 5; ++j) issue(j, j < nun);
  asm volatile("s_waitcnt vmcnt(6)" ::: "memory");  // units 3, 4 (real or dummy) may stay in flight
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  bf16x8 af[5], bfg[7];
  if (nun > 0) {
#pragma unroll
    for (int c = 0; c < 5; ++c) af[c] = tr_read(smem + a_off + c * 32, W2_DYC * 2);
#pragma unroll
    for (int jj = 0; jj < 7; ++jj) bfg[jj] = tr_read(smem + b_off[jj], W2_XC * 2);
    if (bias_col) bfg[6] = ones;
  }
  // one unit; SU = its slot (compile-time), j = its index.  Returns false when the slab is finished.
  auto unit = [&](int j, auto su_c) __attribute__((always_inline)) -> bool {
    constexpr int SU = decltype(su_c)::value, SN = (SU + 1) % 6, S5 = (SU + 5) % 6;
    constexpr bool SYNC = (SU & 1) == 0;  // slots alternate with the unit index: even units synchronise
    if (j >= nun) return false;
    if (SYNC) {
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");     // units j + 1, j + 2 have landed; j + 3, j + 4 (real or dummy) stay in flight
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's reads of unit j are complete
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
    const char* src = smem + ((j + 1 < nun) ? SN : SU) * W3_BUF;  // (last unit: re-read its own slot; the values are not used)
    // units j+5, j+6 -> the slots of units j-1 and j (free since this unit's barrier), as in conv_wgrad3_kernel: h = 0 issues its copies BEFORE
    // its MFMAs, h = 1 after them.  (Issuing one unit's copies in EVERY iteration, or the copy instructions between the MFMA columns, made hipcc
    // spill the accumulators -- 3 KB of scratch per lane, 25x slower; the same happens to conv_wgrad3_kernel with that change alone.)
#ifdef VMG_DIAG
    const bool nocopy = a.dbg & 1;
#else
    constexpr bool nocopy = false;
#endif
    if (SYNC && h == 0) {
      issue(S5, j + 5 < nun && !nocopy);
      issue(SU, j + 6 < nun && !nocopy);
    }
#pragma unroll
    for (int jj = 0; jj < 7; ++jj) {
#ifdef VMG_DIAG
      if (!(a.dbg & 2))
#endif
      {
#pragma unroll
        for (int c = 0; c < 5; ++c) acc[c][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[c], bfg[jj], acc[c][jj], 0, 0, 0);
      }
#ifdef VMG_DIAG
      if (!(a.dbg & 4))
#endif
      if (jj < 6 || !bias_col) bfg[jj] = tr_read(src + b_off[jj], W2_XC * 2);  // (q = 3: column 6 stays the ones operand; a wave-uniform skip of two reads)
    }
#ifdef VMG_DIAG
    if (!(a.dbg & 4))
#endif
    {
#pragma unroll
      for (int c = 0; c < 5; ++c) af[c] = tr_read(src + a_off + c * 32, W2_DYC * 2);  // (behind the last MFMA that reads af[c])
    }
    if (SYNC && h == 1) {
      issue(S5, j + 5 < nun && !nocopy);
      issue(SU, j + 6 < nun && !nocopy);
    }
    return true;
  };
  for (int base = 0; base < nun; base += 6) {
    if (!unit(base + 0, std::integral_constant<int, 0>{})) break;
    if (!unit(base + 1, std::integral_constant<int, 1>{})) break;
    if (!unit(base + 2, std::integral_constant<int, 2>{})) break;
    if (!unit(base + 3, std::integral_constant<int, 3>{})) break;
    if (!unit(base + 4, std::integral_constant<int, 4>{})) break;
    if (!unit(base + 5, std::integral_constant<int, 5>{})) break;
  }
  asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");  // (the dummy copies of the last iterations too: no LDS-DMA outlives the loop)
  // slab store: native accumulator layout, one float4 per lane per tile (fully coalesced)
  float* sl = a.slab + ((((long long)zz * a.gy + blk.y) * a.gx + blk.x) * W3_WAVES + wave) * (W3_TILES * 256);
#pragma unroll
  for (int c = 0; c < 5; ++c)
#pragma unroll
    for (int j = 0; j < 7; ++j) *reinterpret_cast<f32x4*>(sl + ((c * 7 + j) * 64 + lane) * 4) = acc[c][j];
  // (bias: column 6 of the q = 3 waves, see above; slot 35 of the wave's slab stays unused)
}

__global__ __launch_bounds__(256) void conv_wgrad3_reduce_kernel(const float* __restrict__ slab0, int S, int gx, int gy, int Cin, int Cout,
                                                                 const Wgrad3Out outs, int I_total, int o0, int i0, int bias_in_pad) {
  __shared__ float red[256];
  const long long per_s = (long long)gy * gx * W3_WG_FLOATS;
  const float* __restrict__ slab = slab0 + (long long)blockIdx.y * S * per_s;  // blockIdx.y = problem
  float* __restrict__ dW = outs.dW[blockIdx.y];
  float* __restrict__ db = outs.db[blockIdx.y];
  const float scale = outs.scale[blockIdx.y];
  for (long long e0 = blockIdx.x * 64LL; e0 < per_s; e0 += (long long)gridDim.x * 64) {
    const long long i = e0 + (threadIdx.x & 63);
    const float sum = slab_sum_4waves(slab, per_s, S, i, true, red);
    if (threadIdx.x >= 64) continue;
    const int r = (int)(i & 3);
    const int lane = (int)((i >> 2) & 63);
    long long qq = i >> 8;
    const int tile = (int)(qq % W3_TILES);
    qq /= W3_TILES;
    const int wave = (int)(qq % W3_WAVES);
    qq /= W3_WAVES;
    const int coblk = (int)(qq % gx), ciblk = (int)(qq / gx);
    const int h = wave >> 2, q = wave & 3;
    const int g = lane >> 4, l15 = lane & 15;
    if (tile < 35) {
      const int c = tile / 7, j = tile - c * 7;
      const int cot = h * 5 + c, col = q * 7 + j;
      if (cot < 9 && col < 27) {
        const int itile = col / 9, t = col - itile * 9;
        const int co = coblk * W2_DYC + cot * 16 + 4 * g + r;
        const int ci = ciblk * W2_XC + itile * 16 + l15;
        if (co < Cout && ci < Cin) dW[((long long)(o0 + co) * I_total + (i0 + ci)) * 9 + t] += sum * scale;
      }
    } else if (!bias_in_pad && db && q == 0 && ciblk == 0 && l15 < 5) {
      const int cot = h * 5 + l15;
      const int co = coblk * W2_DYC + cot * 16 + 4 * g + r;
      if (cot < 9 && co < Cout) db[o0 + co] += sum * scale;
    }
    if (bias_in_pad && db && tile < 35 && q == 3 && ciblk == 0 && l15 == 0 && tile % 7 == 6) {  // conv_wgrad3b_kernel: the padding column of the q = 3 waves
      const int cot = h * 5 + tile / 7;
      const int co = coblk * W2_DYC + cot * 16 + 4 * g + r;
      if (cot < 9 && co < Cout) db[o0 + co] += sum * scale;
    }
  }
}

// =====================================================================================================
// v2 for 1x1 convolutions / Linears (bf16): dW[co][ci] = sum_p dY[p][co] * X[p][ci], a GEMM whose K is the pixel list.
// Workgroup = 9 waves (cg, it); output tile 144 co x 144 ci, wave (cg, it) owns co tiles 3cg..3cg+2 x ci tiles 3it..3it+2
// (9 accumulator tiles + the bias tile for it == 0).  A unit = 32 consecutive pixels of the flat pixel list: both tiles
// ([32][144] bf16, 9 KiB each) arrive by LDS-DMA exactly as they lie in HBM, one 16-byte vector per thread and tile, and
// are read TRANSPOSED (ds_read_b64_tr_b16).  Three LDS buffers, one barrier per unit: at the top of iteration u a wave waits for its own share of unit u, and the
// barrier also tells it that nobody reads unit u-1's buffer any more, so unit u+2 may overwrite it; the LDS
// footprint (54 KiB) and register use allow two workgroups per CU, whose barrier bubbles overlap.  The pixel list is
// cut into S slabs; partial tiles go to the workspace and the reduce kernel adds them to dW in slab order.
struct Lgrad2K {
  const char* x[W3_MAX_PROBS * WG_MAX_PAIRS];   // [problem][pair]
  const char* dy[W3_MAX_PROBS * WG_MAX_PAIRS];
  int npairs, nprob;
  long long Mpair;   // pixels per pair
  long long Upair, U;  // 32-pixel units per pair / in total
  long long x_ps, dy_ps;
  int Cin, Cout;
  float* slab;  // [problem][S][ciblk][coblk][9 waves][10 tiles][64][4]
  int S, has_bias;
  int gx, gy;   // co / ci blocks (1-D grid of gx * gy * S workgroups, see xcd_slab_block)
};
constexpr int L2_TILE_BYTES = 32 * 144 * 2;  // 9216
constexpr int L2_BUF = 2 * L2_TILE_BYTES;    // dY tile + X tile
constexpr int L2_TILES = 10;
constexpr long long L2_WG_FLOATS = (long long)W2_WAVES * L2_TILES * 256;

__global__ __launch_bounds__(W2_THREADS, 2) void linear_wgrad2_kernel(const Lgrad2K a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cg = wave / 3, it = wave - cg * 3;
  SlabBlock blk = xcd_slab_block(a.gx, a.gy, a.S * a.nprob);
  const int prob = blk.z / a.S, zz = blk.z;  // (several problems of one shape per launch, as in conv_wgrad3_kernel)
  blk.z -= prob * a.S;
  const char* const* xs = a.x + prob * WG_MAX_PAIRS;
  const char* const* dys = a.dy + prob * WG_MAX_PAIRS;
  const int ob = blk.x * 144, ib = blk.y * 144;
  const long long u_lo = a.U * blk.z / a.S, u_hi = a.U * (blk.z + 1) / a.S;
  const char* zsrc = reinterpret_cast<const char*>(g_zero_buf);

  f32x4 acc[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[c][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 accb[3] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  const bf16 one = (bf16)1.0f;
  const bf16x8 ones = {one, one, one, one, one, one, one, one};

  // lane constants: thread tid moves vector v (8 channels) of pixel p of both tiles
  const int p_l = tid / 18, v_l = tid - p_l * 18;
  const bool c_dy = ob + v_l * 8 + 8 <= a.Cout, c_x = ib + v_l * 8 + 8 <= a.Cin;
  const int off_dy = (int)((p_l * a.dy_ps + ob + v_l * 8) * 2), off_x = (int)((p_l * a.x_ps + ib + v_l * 8) * 2);
  int ipair = (int)(u_lo / a.Upair);
  long long ipix = (u_lo - (long long)ipair * a.Upair) * 32;  // first pixel (within the pair) of the unit to issue next
  auto issue = [&](int buf) {
    const bool pok = ipix + p_l < a.Mpair;
    char* dyt = smem + buf * L2_BUF;
    const char* s0 = (pok && c_dy) ? dys[ipair] + ipix * a.dy_ps * 2 + off_dy : zsrc;
    glds16_hidden(s0, dyt + wave * 1024);
    const char* s1 = (pok && c_x) ? xs[ipair] + ipix * a.x_ps * 2 + off_x : zsrc;
    glds16_hidden(s1, dyt + L2_TILE_BYTES + wave * 1024);
    ipix += 32;
    if (ipix >= a.Mpair) { ipix = 0; ++ipair; }
  };

  if (u_lo < u_hi) issue(0);
  if (u_lo + 1 < u_hi) issue(1);
  int buf = 0;
  for (long long u = u_lo; u < u_hi; ++u) {
    if (u + 1 < u_hi) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");  // unit u landed; unit u+1 (2 instructions per wave) stays in flight
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const char* dyt = smem + buf * L2_BUF;
    const char* xt = dyt + L2_TILE_BYTES;
    bf16x8 af[3], bfg[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) af[c] = tr_frag(dyt, 288, 0, (cg * 3 + c) * 16, lane);
#pragma unroll
    for (int j = 0; j < 3; ++j) bfg[j] = tr_frag(xt, 288, 0, (it * 3 + j) * 16, lane);
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[c], bfg[j], acc[c][j], 0, 0, 0);
    if (a.has_bias && it == 0 && blk.y == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) accb[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[c], ones, accb[c], 0, 0, 0);
    }
    if (u + 2 < u_hi) issue(buf == 0 ? 2 : buf - 1);  // (behind the MFMAs: the copy's address arithmetic runs in their shadow)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    buf = buf == 2 ? 0 : buf + 1;
  }
  float* sl = a.slab + ((((long long)zz * a.gy + blk.y) * a.gx + blk.x) * W2_WAVES + wave) * (L2_TILES * 256);
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int j = 0; j < 3; ++j) *reinterpret_cast<f32x4*>(sl + ((c * 3 + j) * 64 + lane) * 4) = acc[c][j];
  if (a.has_bias && it == 0 && blk.y == 0) {
    f32x4 pack = f32x4{0.f, 0.f, 0.f, 0.f};
    const int l15 = lane & 15;
    if (l15 < 3) pack = l15 == 0 ? accb[0] : (l15 == 1 ? accb[1] : accb[2]);
    *reinterpret_cast<f32x4*>(sl + (9 * 64 + lane) * 4) = pack;
  }
}

__global__ __launch_bounds__(256) void linear_wgrad2_reduce_kernel(const float* __restrict__ slab0, int S, int gx, int gy, int Cin, int Cout,
                                                                   const Wgrad3Out outs, int I_total, int o0, int i0) {
  __shared__ float red[256];
  const long long per_s = (long long)gy * gx * L2_WG_FLOATS;
  const float* __restrict__ slab = slab0 + (long long)blockIdx.y * S * per_s;  // blockIdx.y = problem
  float* __restrict__ dW = outs.dW[blockIdx.y];
  float* __restrict__ db = outs.db[blockIdx.y];
  const float scale = outs.scale[blockIdx.y];
  for (long long e0 = blockIdx.x * 64LL; e0 < per_s; e0 += (long long)gridDim.x * 64) {
    const long long i = e0 + (threadIdx.x & 63);
    const float sum = slab_sum_4waves(slab, per_s, S, i, true, red);
    if (threadIdx.x >= 64) continue;
    const int r = (int)(i & 3);
    const int lane = (int)((i >> 2) & 63);
    long long q = i >> 8;
    const int tile = (int)(q % L2_TILES);
    q /= L2_TILES;
    const int wave = (int)(q % W2_WAVES);
    q /= W2_WAVES;
    const int coblk = (int)(q % gx), ciblk = (int)(q / gx);
    const int cg = wave / 3, it = wave - cg * 3;
    const int g = lane >> 4, l15 = lane & 15;
    if (tile < 9) {
      const int c = tile / 3, j = tile - c * 3;
      const int co = coblk * 144 + (cg * 3 + c) * 16 + 4 * g + r;
      const int ci = ciblk * 144 + (it * 3 + j) * 16 + l15;
      if (co < Cout && ci < Cin) dW[(long long)(o0 + co) * I_total + (i0 + ci)] += sum * scale;
    } else if (db && it == 0 && ciblk == 0 && l15 < 3) {
      const int co = coblk * 144 + (cg * 3 + l15) * 16 + 4 * g + r;
      if (co < Cout) db[o0 + co] += sum * scale;
    }
  }
}

// =====================================================================================================
// 7x7 (SPyNet's ConvModules, reference models/vmg.py:126-173), bf16: dW[co][ci][ky][kx] = sum_p dY[p][co] * X[p + (ky-3, kx-3)][ci].
// Workgroup = SEVEN waves, wave ky owns tap row ky: CT output-channel tiles x 7 kx = 7*CT accumulator tiles of one 16-channel ci
// block (grid.x = ci blocks, grid.y = K slabs).  A K unit = W7_R image rows x 32 pixels: the dY tile (R x 32 pixels x CT*16
// channels) and the X tile with its 3-pixel halo ((R + 6) x 38 pixels x 16 channels) are fetched by all 448 threads with
// UNCONDITIONAL 16-byte loads (lanes outside the image / past the channels read a zero buffer) one unit ahead into registers,
// written to one of two LDS buffers, one barrier per unit.  Per image row a wave reads CT dY fragments and 7 X fragments (the
// same staged row serves all kx: the fragment's first pixel is kx) transposed with ds_read_b64_tr_b16 for 7*CT MFMAs.  Every
// (co, ci, tap) lives in exactly one wave: no reduction inside the workgroup; slab partials in the accumulators' native layout
// (coalesced float4 stores) and a second kernel sums the slabs in a fixed order (deterministic) into dW / db.  The bias
// gradient is one more MFMA per co tile against a ones vector on wave 0 of ci block 0.
// The same kernel with KS = 3 (three waves, 8 rows per unit) takes the 3x3 convs with <= 16 output channels (conv_last: 64 -> 3 on the 1.8 M
// HR pixels of a batch), where the 144-channel tile of conv_wgrad3_kernel would be 9/10 padding.
constexpr int W7_X_RS = 48;  // LDS pixel stride of the X tile: 16 channels + 16 bytes (conflict-free transposed reads)
template <int KS>
struct W7Geo {
  static constexpr int R = KS == 7 ? 4 : 8;  // image rows per K unit (3x3 with 4 rows and 768 workgroups: 140 us instead of 122 on conv_last)
  static constexpr int THREADS = KS * 64, XW = 32 + KS - 1, XR = R + KS - 1;
  static constexpr int XVEC = XR * XW * 2;  // 16-byte vectors of the X tile (7x7: 760)
  static constexpr int NX = (XVEC + THREADS - 1) / THREADS;
  static constexpr int X_BYTES = ((NX * THREADS + 1) / 2) * W7_X_RS;  // room for every thread's NX vectors: the staging stores are unconditional
};
template <int CT, int KS = 7>
struct W7Cfg {
  using G = W7Geo<KS>;
  static constexpr int DY_RS = CT * 32 + 16, DYVEC = G::R * 32 * CT * 2;
  static constexpr int NX = G::NX, NDY = (DYVEC + G::THREADS - 1) / G::THREADS;
  static constexpr int DY_BYTES = ((NDY * G::THREADS + CT * 2 - 1) / (CT * 2)) * DY_RS;  // (same: room for the padding vectors)
  static constexpr int BUF = (G::X_BYTES + DY_BYTES + 15) & ~15;
  static constexpr int WG_FLOATS = (KS * KS * CT + CT) * 256;  // tiles [ky][ct][kx], then the CT bias tiles
};

struct Wgrad7K {
  const char* x[WG_MAX_PAIRS];
  const char* dy[WG_MAX_PAIRS];
  int npairs;
  int Upair, U;       // K units per pair / in total
  long long x_ps, dy_ps;
  int Cin, Cout;      // true channel counts
  int vec_dy;         // dY can be read as 16-byte vectors (else element by element: the 2-channel flow head)
  float* slab;        // [S][ci blocks][WG_FLOATS]
  int N, H, W, SEG, HB, S;
  int has_bias;
  int gx;             // ci blocks (1-D grid of gx * S workgroups, see xcd_slab_block)
};

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
template <int CT, int KS>
__global__ __launch_bounds__(W7Geo<KS>::THREADS) void conv_wgrad7_kernel(const Wgrad7K a) {
  using C = W7Cfg<CT, KS>;
  using G = W7Geo<KS>;
  constexpr int W7_THREADS = G::THREADS, W7_XW = G::XW, W7_XVEC = G::XVEC, W7_X_BYTES = G::X_BYTES, W7_RU = G::R, HALO = KS / 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int ky = __builtin_amdgcn_readfirstlane(tid >> 6);
  const SlabBlock blk = xcd_slab_block(a.gx, 1, a.S);
  const int ib = blk.x * 16;
  const int u_lo = (int)((long long)a.U * blk.z / a.S), u_hi = (int)((long long)a.U * (blk.z + 1) / a.S);
  const bool do_bias = a.has_bias && blk.x == 0 && ky == 0;
  const char* zsrc = reinterpret_cast<const char*>(g_zero_buf);

  f32x4 acc[CT][KS], accb[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    accb[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kx = 0; kx < KS; ++kx) acc[ct][kx] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const __bf16 one = (__bf16)1.0f;
  const bf16x8 ones = {one, one, one, one, one, one, one, one};

  u32x4 rx[C::NX], rdy[C::NDY];  // (a native vector type: the HIP uint4 struct is copied with memcpy and stays in scratch)
  auto fetch = [&](int ug) __attribute__((always_inline)) {
    const int pair = ug / a.Upair;
    int u = ug - pair * a.Upair;
    const int seg = u % a.SEG;
    u /= a.SEG;
    const int hb = u % a.HB, n = u / a.HB;
    const int y0 = hb * W7_RU, x0 = seg * 32;
    const char* xb = a.x[pair];
    const char* db_ = a.dy[pair];
#pragma unroll
    for (int k = 0; k < C::NX; ++k) {
      const int idx = tid + k * W7_THREADS;
      const int pp = idx >> 1, v = idx & 1;
      const int r = pp / W7_XW, col = pp - r * W7_XW;
      const int yy = y0 + r - HALO, xx = x0 + col - HALO, c = ib + v * 8;
      const bool ok = idx < W7_XVEC && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W && c + 8 <= a.Cin;
      const long long off = ((((long long)n * a.H + yy) * a.W + xx) * a.x_ps + c) * 2;
      rx[k] = *reinterpret_cast<const u32x4*>(ok ? xb + off : zsrc);
    }
    if (a.vec_dy) {
#pragma unroll
      for (int k = 0; k < C::NDY; ++k) {
        const int idx = tid + k * W7_THREADS;
        const int pp = idx / (CT * 2), v = idx - pp * (CT * 2);
        const int rr = pp >> 5, col = pp & 31;
        const bool ok = idx < C::DYVEC && y0 + rr < a.H && x0 + col < a.W && v * 8 < a.Cout;  // (a vector that starts inside the channels ends inside the pixel stride)
        const long long off = ((((long long)n * a.H + y0 + rr) * a.W + x0 + col) * a.dy_ps + v * 8) * 2;
        rdy[k] = *reinterpret_cast<const u32x4*>(ok ? db_ + off : zsrc);
      }
    } else {
#pragma unroll
      for (int k = 0; k < C::NDY; ++k) {
        const int idx = tid + k * W7_THREADS;
        const int pp = idx / (CT * 2), v = idx - pp * (CT * 2);
        const int rr = pp >> 5, col = pp & 31;
        const bool ok = idx < C::DYVEC && y0 + rr < a.H && x0 + col < a.W;
        const long long off = ((((long long)n * a.H + y0 + rr) * a.W + x0 + col) * a.dy_ps + v * 8) * 2;
        unsigned short tmp[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) tmp[e] = *reinterpret_cast<const unsigned short*>((ok && v * 8 + e < a.Cout) ? db_ + off + 2 * e : zsrc);
        rdy[k] = u32x4{tmp[0] | (unsigned)tmp[1] << 16, tmp[2] | (unsigned)tmp[3] << 16, tmp[4] | (unsigned)tmp[5] << 16, tmp[6] | (unsigned)tmp[7] << 16};
      }
    }
  };
  auto stage = [&](char* buf) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < C::NX; ++k) {
      const int idx = tid + k * W7_THREADS;
      *reinterpret_cast<u32x4*>(buf + (idx >> 1) * W7_X_RS + (idx & 1) * 16) = rx[k];
    }
#pragma unroll
    for (int k = 0; k < C::NDY; ++k) {
      const int idx = tid + k * W7_THREADS;
      const int pp = idx / (CT * 2), v = idx - pp * (CT * 2);
      *reinterpret_cast<u32x4*>(buf + W7_X_BYTES + pp * C::DY_RS + v * 16) = rdy[k];
    }
  };

  int which = 0;
  if (u_lo < u_hi) fetch(u_lo);
  for (int u = u_lo; u < u_hi; ++u) {
    char* buf = smem + which * C::BUF;
    stage(buf);
    __syncthreads();  // the unit is complete in `buf`; every wave has finished the unit before the previous one (the other buffer is free again after the NEXT barrier)
    if (u + 1 < u_hi) fetch(u + 1);
    const char* xt = buf;
    const char* dyt = buf + W7_X_BYTES;
#pragma unroll
    for (int rr = 0; rr < W7_RU; ++rr) {
      bf16x8 af[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) af[ct] = tr_frag(dyt, C::DY_RS, rr * 32, ct * 16, lane);
      const char* xrow = xt + (rr + ky) * (W7_XW * W7_X_RS);
#pragma unroll
      for (int kx = 0; kx < KS; ++kx) {
        const bf16x8 bfg = tr_frag(xrow, W7_X_RS, kx, 0, lane);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[ct][kx] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ct], bfg, acc[ct][kx], 0, 0, 0);
      }
      if (do_bias) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) accb[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ct], ones, accb[ct], 0, 0, 0);
      }
    }
    which ^= 1;
  }

  float* sl = a.slab + ((long long)blk.z * a.gx + blk.x) * C::WG_FLOATS;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int kx = 0; kx < KS; ++kx)
      *reinterpret_cast<f32x4*>(sl + (((ky * CT + ct) * KS + kx) * 64 + lane) * 4) = acc[ct][kx];
  if (ky == 0) {  // (written by every ci block so that the reduce kernel never reads uninitialised memory)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) *reinterpret_cast<f32x4*>(sl + ((KS * KS * CT + ct) * 64 + lane) * 4) = accb[ct];
  }
}

__global__ __launch_bounds__(256) void conv_wgrad7_reduce_kernel(const float* __restrict__ slab, int S, int gx, int CT, int KS, int Cin, int Cout,
                                                                 float* __restrict__ dW, int I_total, int o0, int i0,
                                                                 float* __restrict__ db, float scale) {
  __shared__ float red[256];
  const int KK = KS * KS, wgf = (KK * CT + CT) * 256;
  const long long per_s = (long long)gx * wgf;
  for (long long e0 = blockIdx.x * 64LL; e0 < per_s; e0 += (long long)gridDim.x * 64) {
    const long long i = e0 + (threadIdx.x & 63);
    const float sum = slab_sum_4waves(slab, per_s, S, i, true, red);
    if (threadIdx.x >= 64) continue;
    const int ciblk = (int)(i / wgf);
    const int e = (int)(i - (long long)ciblk * wgf);
    const int r = e & 3, lane = (e >> 2) & 63, tile = e >> 8;
    const int g = lane >> 4, l15 = lane & 15;
    if (tile < KK * CT) {
      const int kx = tile % KS, ct = (tile / KS) % CT, ky = tile / (KS * CT);
      const int co = ct * 16 + 4 * g + r, ci = ciblk * 16 + l15;
      if (co < Cout && ci < Cin) dW[((long long)(o0 + co) * I_total + (i0 + ci)) * KK + ky * KS + kx] += sum * scale;
    } else if (db && ciblk == 0 && l15 == 0) {
      const int co = (tile - KK * CT) * 16 + 4 * g + r;
      if (co < Cout) db[o0 + co] += sum * scale;
    }
  }
}

// =====================================================================================================
// Host side.  Every entry point fills one WgradCall, then: wgrad_validate (the hard errors) -> wgrad_plan (which kernel, which grid;
// a pure function of integers, also exported as vmg_conv_wgrad_plan) -> wgrad_launch (fills the kernel's argument struct and launches).
// =====================================================================================================
constexpr int WG_NULL = 8;  // beside the VMG_WGRAD_ALIGN_* facts: a pointer the entry needs is null

struct WgradCall {
  int entry, dtype, ks, nprob, npairs;
  const void* const* x;   // [problem][pair]
  const void* const* dy;
  int N, H, W;            // (0 from vmg_linear_wgrad2_multi, which knows only M)
  long long M;            // pixels per pair
  long long x_ps, dy_ps;
  int Cin, Cout;
  float* const* dW;       // per problem
  float* const* db;       // per problem; the table or an entry may be null
  const float* scale;     // per problem
  int I_total, o0, i0;
  void* ws;
  long long ws_bytes;     // 0 without a workspace
};

struct WgradPlan {
  int kernel;       // as vmg_conv_wgrad_last_kernel reports it; 0: the large-tile kernel of a multi entry does not apply
  int gx, gy, S;    // co blocks, ci blocks, K splits
  long long wgs;    // workgroups of the main launch
  int slabs;        // 1: partial sums to the workspace and a reduce kernel, 0: float atomics
  int rblocks;      // blocks of the reduce launch (x nprob)
};

long long pixels(int N, int H, int W) { return N > 0 && H > 0 && W > 0 ? (long long)N * H * W : 0; }

// Alignment facts of a call's pointers, WG_NULL if one is missing.  (Counts out of range: nothing is read, wgrad_validate rejects the call.)
int wgrad_pointer_facts(const WgradCall& d) {
  if (!d.x || !d.dy || !d.dW || !d.scale || (d.entry == VMG_WGRAD_ENTRY_MULTI && !d.ws)) return WG_NULL;
  if (d.nprob < 1 || d.nprob > W3_MAX_PROBS || d.npairs < 1 || d.npairs > WG_MAX_PAIRS) return 0;
  int f = VMG_WGRAD_ALIGN_X16 | VMG_WGRAD_ALIGN_DY16 | VMG_WGRAD_ALIGN_DY2;
  for (int p = 0; p < d.nprob * d.npairs; ++p) {
    if (!d.x[p] || !d.dy[p]) return WG_NULL;
    if ((uintptr_t)d.x[p] % 16) f &= ~VMG_WGRAD_ALIGN_X16;
    if ((uintptr_t)d.dy[p] % 16) f &= ~VMG_WGRAD_ALIGN_DY16;
    if ((uintptr_t)d.dy[p] % 2) f &= ~VMG_WGRAD_ALIGN_DY2;
  }
  for (int q = 0; q < d.nprob; ++q)
    if (!d.dW[q]) return WG_NULL;
  return f;
}

// The hard errors.  What only keeps a problem from a fast kernel is none: wgrad_plan then picks the general kernel, or no kernel for
// the multi entries, which have no general kernel to fall back to and fail.
int wgrad_validate(const WgradCall& d, int facts) {
  const bool multi = d.entry == VMG_WGRAD_ENTRY_MULTI;
  VMG_CHECK(d.ks == 1 || d.ks == 3 || d.ks == 7, "conv_wgrad: ks must be 1, 3 or 7");
  VMG_CHECK(d.dtype == VMG_F32 || d.dtype == VMG_BF16, "conv_wgrad: bad dtype");
  VMG_CHECK(d.M > 0 && d.Cin > 0 && d.Cout > 0, "conv_wgrad: bad shape");
  VMG_CHECK(d.nprob >= 1 && d.nprob <= (multi ? W3_MAX_PROBS : 1) && d.npairs >= 1 && d.npairs <= WG_MAX_PAIRS, "conv_wgrad: 1..%d problems, 1..%d (x, dy) pairs",
            W3_MAX_PROBS, WG_MAX_PAIRS);
  VMG_CHECK(!(facts & WG_NULL), "conv_wgrad: null pointer");
  VMG_CHECK(d.x_ps >= d.Cin && d.dy_ps >= d.Cout && d.i0 >= 0 && d.i0 + d.Cin <= d.I_total && d.o0 >= 0, "conv_wgrad: bad strides / slices");
  return 0;
}

constexpr int w7_ct(int ks, int Cout) { return ks == 3 || Cout <= 16 ? 1 : Cout <= 32 ? 2 : 4; }
constexpr long long w7_wg_floats(int ks, int ct) { return (long long)(ks * ks * ct + ct) * 256; }
constexpr long long reduce_blocks(long long elems, int per_block, int most) { return (elems + per_block - 1) / per_block > most ? most : (elems + per_block - 1) / per_block; }

// Which kernel serves the call, and with which grid.  Pure: integers in, integers out (variant = g_w3_variant).  Rules in order; all
// divisions are integer divisions.
WgradPlan wgrad_plan(const WgradCall& d, int variant, int facts) {
  const bool multi = d.entry == VMG_WGRAD_ENTRY_MULTI, bf = d.dtype == VMG_BF16;
  const bool x16 = facts & VMG_WGRAD_ALIGN_X16, dy16 = facts & VMG_WGRAD_ALIGN_DY16, dy2 = facts & VMG_WGRAD_ALIGN_DY2;
  const bool xs8 = d.x_ps % 8 == 0, dys8 = d.dy_ps % 8 == 0;
  const long long ws_bytes = d.entry == VMG_WGRAD_ENTRY_PLAIN ? 0 : d.ws_bytes;  // (0: no rule below finds room for a slab)
  const int seg = cdiv(d.W, 32);
  WgradPlan p = {};
  auto slabs = [&p](int kernel, long long S, long long groups, long long slab) {  // groups: workgroups, slab: floats, both per K split (and problem)
    p.kernel = kernel; p.S = (int)S; p.wgs = groups * S; p.slabs = 1; p.rblocks = (int)reduce_blocks(slab, 64, 8192);
    return p;
  };
  // 1. 1x1 large tile (linear_wgrad2_kernel): every channel count and stride in whole 16-byte vectors, at least 64 units of 32 pixels
  //    (fewer: the general kernel's single launch is cheaper)
  if (bf && d.ks == 1 && xs8 && dys8 && d.Cin % 8 == 0 && d.Cout % 8 == 0 && x16 && dy16) {
    const long long U = cdiv64(d.M, 32) * d.npairs;
    p.gx = cdiv(d.Cout, 144); p.gy = cdiv(d.Cin, 144);
    const long long groups = (long long)p.gx * p.gy * d.nprob, slab = p.gx * p.gy * L2_WG_FLOATS;
    const long long S = std::max(1LL, std::min(512 / groups, U / 8));  // two workgroups per CU over all problems
    if (U >= 64 && d.nprob * S * slab * 4 <= ws_bytes) return slabs(last_kernel_id(VMG_WGRAD_L2), S, groups, slab);
  }
  // 2. one wave per tap row (conv_wgrad7_kernel): 7x7 with <= 64 output channels, 3x3 with <= 16 (the 144-channel tile would be 9/10
  //    padding).  dY may be unaligned and of any stride (then read element by element: the 2-channel flow head); channels of X past
  //    Cin would be multiplied, so Cin itself is a multiple of 8
  if (!multi && bf && ((d.ks == 7 && d.Cout <= 64) || (d.ks == 3 && d.Cout <= 16)) && xs8 && d.Cin % 8 == 0 && x16 && dy2) {
    const long long U = (long long)d.npairs * d.N * cdiv(d.H, d.ks == 7 ? W7Geo<7>::R : W7Geo<3>::R) * seg;
    const int ct = w7_ct(d.ks, d.Cout);
    p.gx = cdiv(d.Cin, 16); p.gy = 1;
    const long long slab = p.gx * w7_wg_floats(d.ks, ct), cap = ws_bytes / (slab * 4);
    // ~two rounds of workgroups over the 256 CUs, >= 2 units each
    if (U < (1LL << 30) && cap >= 1) return slabs(last_kernel_id(VMG_WGRAD_7, ct, d.ks), std::max(1LL, std::min({512LL / p.gx, U / 2, cap})), p.gx, slab);
  }
  // 3. 3x3 large tile: 8-channel vectors that may run past the channel count when the pixel stride has room for the whole last vector
  //    (the zero-padded input of the 3-channel stem conv, a slice of a wider tensor: the extra channels are computed and dropped)
  if (bf && d.ks == 3 && (multi || d.Cout > 16) && xs8 && dys8 && d.x_ps >= ((d.Cin + 7) & ~7) && d.dy_ps >= ((d.Cout + 7) & ~7) && x16 && dy16) {
    const long long U = (long long)d.N * d.H * seg * d.npairs;
    p.gx = cdiv(d.Cout, W2_DYC); p.gy = cdiv(d.Cin, W2_XC);
    const long long groups = (long long)p.gx * p.gy * d.nprob, slab = p.gx * p.gy * W3_WG_FLOATS;
    const long long S = std::max(1LL, std::min(256 / groups, U / 8));  // one workgroup per CU over all problems
    // the buffer-addressed variant needs every byte of a pair's tensors (plus the X tile's reach of two rows and 34 pixels) below 2^31 from the base
    const long long reach = (d.M + 2LL * d.W + 40) * std::max(d.x_ps, d.dy_ps) * 2;
    if (d.nprob * S * slab * 4 <= ws_bytes) return slabs(last_kernel_id(variant == 1 && reach < (1LL << 31) ? VMG_WGRAD_3B : VMG_WGRAD_3), S, groups, slab);
  }
  if (multi) return WgradPlan{};  // (no large-tile kernel: the entry fails)
  // 4. the general kernel.  bf16 3x3 with <= 16 output channels: one co tile, and 64 input channels per workgroup (whole 128-byte pixel
  //    rows of X) when there are that many.  Float atomics, except 7x7 with a workspace of >= 1 MiB: 49 taps x one 16 x 16 tile per
  //    workgroup, few (co, ci) tiles and many K splits, whose atomics would all hit the same few addresses
  const int small3 = bf && d.ks == 3 && d.Cout <= 16;
  const int ct = d.ks == 7 || small3 ? 1 : 3, it = d.ks == 1 ? 3 : small3 && d.Cin >= 64 ? 4 : 1;
  const long long U = (d.ks > 1 ? (long long)d.N * d.H * seg : cdiv64(d.M, 32)) * d.npairs;
  p.gx = cdiv(d.Cout, ct * 16); p.gy = cdiv(d.Cin, it * 16);
  const long long slab = (long long)p.gx * p.gy * (ct * 16 * it * 16 * d.ks * d.ks + ct * 16), ws_floats = ws_bytes / 4;  // slab: floats of one K split
  long long S = std::min(1024 / ((long long)p.gx * p.gy), U / 32);  // ~4 workgroups per CU in flight; >= 8 K units per wave, or the epilogue dominates
  p.slabs = d.ks == 7 && ws_bytes >= (1 << 20);
  if (p.slabs) S = std::min(S, ws_floats / slab);
  S = std::max(1LL, std::min(S, 65535LL));
  if (p.slabs && S * slab > ws_floats) p.slabs = 0;  // (not even one split fits)
  p.kernel = last_kernel_id(VMG_WGRAD_V1, d.ks, ct, it); p.S = (int)S; p.wgs = p.gx * p.gy * S;
  p.rblocks = p.slabs ? (int)reduce_blocks(slab, 256, 4096) : 0;
  return p;
}

// The dynamic-LDS limit of a kernel, set once per kernel and device.
template <auto Kernel>
void allow_lds(int bytes) {
  static bool done[VMG_MAX_DEVICES] = {};
  const int dev = vmg_current_device();
  if (done[dev]) return;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  done[dev] = true;
}

template <typename T, int KS, int CT, int IT>
int launch_v1(const WgradCall& d, const WgradPlan& p, int facts, hipStream_t st) {
  using C = WgradCfg<T, KS, CT, IT>;
  static_assert(C::LDS_BYTES <= 160 * 1024, "wgrad LDS");
  WgradK k;
  memset(&k, 0, sizeof(k));
  // 16-byte vector loads need a pixel stride that is a multiple of the vector (then a vector that starts inside the channel range ends
  // inside the pixel's stride: a zero-padded or wider tensor behind a channel slice, e.g. the 3-channel output gradient of conv_last
  // padded to 8) and aligned bases; channel counts need not be multiples of 8
  k.vec_x = d.x_ps % C::VPL == 0 && (facts & VMG_WGRAD_ALIGN_X16);
  k.vec_dy = d.dy_ps % C::VPL == 0 && (facts & VMG_WGRAD_ALIGN_DY16);
  for (int i = 0; i < d.npairs; ++i) { k.x[i] = (const char*)d.x[i]; k.dy[i] = (const char*)d.dy[i]; }
  k.npairs = d.npairs;
  k.x_ps = d.x_ps; k.Cin = d.Cin; k.dy_ps = d.dy_ps; k.Cout = d.Cout;
  k.dW = d.dW[0]; k.I_total = d.I_total; k.o0 = d.o0; k.i0 = d.i0; k.db = d.db ? d.db[0] : nullptr; k.scale = d.scale[0];
  k.N = d.N; k.H = d.H; k.W = d.W; k.M = d.M;
  k.SEG = cdiv(d.W, 32);
  k.HB = d.H;  // one row per K unit (2 and 4 rows spilled registers in the 49-tap instantiations)
  k.Upair = KS > 1 ? (long long)d.N * k.HB * k.SEG : cdiv64(k.M, 32);
  k.U = k.Upair * d.npairs;
  k.S = p.S;
  k.slab = p.slabs ? (float*)d.ws : nullptr;
  allow_lds<conv_wgrad_kernel<T, KS, CT, IT>>(160 * 1024);
  hipLaunchKernelGGL((conv_wgrad_kernel<T, KS, CT, IT>), dim3(p.gx, p.gy, p.S), dim3(256), C::LDS_BYTES, st, k);
  VMG_LAUNCH_CHECK();
  if (p.slabs) {
    hipLaunchKernelGGL(wgrad_slab_reduce_kernel, dim3(p.rblocks), dim3(256), 0, st, (const float*)k.slab, k.S, p.gx, p.gy, C::DYC, C::XC, C::KK, k.Cout, k.Cin, k.dW,
                       k.I_total, k.o0, k.i0, k.db, k.scale);
    VMG_LAUNCH_CHECK();
  }
  return 0;
}

template <int CT, int KS>
int launch_w7(const WgradCall& d, const WgradPlan& p, int facts, hipStream_t st) {
  using C = W7Cfg<CT, KS>;
  static_assert(C::WG_FLOATS == w7_wg_floats(KS, CT), "wgrad_plan sizes the tap-row kernel's slabs");
  Wgrad7K k;
  memset(&k, 0, sizeof(k));
  for (int i = 0; i < d.npairs; ++i) { k.x[i] = (const char*)d.x[i]; k.dy[i] = (const char*)d.dy[i]; }
  k.npairs = d.npairs; k.x_ps = d.x_ps; k.dy_ps = d.dy_ps; k.Cin = d.Cin; k.Cout = d.Cout; k.slab = (float*)d.ws;
  k.vec_dy = d.dy_ps % 8 == 0 && (facts & VMG_WGRAD_ALIGN_DY16);  // (channels past Cout inside the last vector are computed and dropped)
  k.N = d.N; k.H = d.H; k.W = d.W; k.SEG = cdiv(d.W, 32); k.HB = cdiv(d.H, W7Geo<KS>::R);
  k.Upair = d.N * k.HB * k.SEG; k.U = k.Upair * d.npairs;
  k.has_bias = d.db && d.db[0];
  k.S = p.S; k.gx = p.gx;
  allow_lds<conv_wgrad7_kernel<CT, KS>>(2 * C::BUF);
  hipLaunchKernelGGL((conv_wgrad7_kernel<CT, KS>), dim3((unsigned)p.wgs), dim3(W7Geo<KS>::THREADS), 2 * C::BUF, st, k);
  VMG_LAUNCH_CHECK();
  hipLaunchKernelGGL(conv_wgrad7_reduce_kernel, dim3(p.rblocks), dim3(256), 0, st, (const float*)k.slab, p.S, p.gx, CT, KS, k.Cin, k.Cout, d.dW[0], d.I_total, d.o0,
                     d.i0, d.db ? d.db[0] : nullptr, d.scale[0]);
  VMG_LAUNCH_CHECK();
  return 0;
}

// What Wgrad2K and Lgrad2K share: the [problem][pair] pointer table, the counts and strides, the plan's grid; and the reduce kernel's outputs.
template <typename K>
void fill_problems(K& k, Wgrad3Out& outs, const WgradCall& d, const WgradPlan& p) {
  memset(&k, 0, sizeof(k));
  memset(&outs, 0, sizeof(outs));
  for (int q = 0; q < d.nprob; ++q) {
    for (int i = 0; i < d.npairs; ++i) {
      k.x[q * WG_MAX_PAIRS + i] = (const char*)d.x[q * d.npairs + i];
      k.dy[q * WG_MAX_PAIRS + i] = (const char*)d.dy[q * d.npairs + i];
    }
    outs.dW[q] = d.dW[q];
    outs.db[q] = d.db ? d.db[q] : nullptr;
    outs.scale[q] = d.scale[q];
    k.has_bias = k.has_bias || outs.db[q] != nullptr;
  }
  k.npairs = d.npairs; k.nprob = d.nprob; k.x_ps = d.x_ps; k.dy_ps = d.dy_ps;
  k.S = p.S; k.slab = (float*)d.ws; k.gx = p.gx; k.gy = p.gy;
}

int launch_w3(const WgradCall& d, const WgradPlan& p, hipStream_t st) {
  Wgrad2K k;
  Wgrad3Out outs;
  fill_problems(k, outs, d, p);
  k.Cin = (d.Cin + 7) & ~7; k.Cout = (d.Cout + 7) & ~7;  // bounds of the 8-channel vector loads; the reduce kernel keeps the true counts
  k.N = d.N; k.H = d.H; k.W = d.W; k.SEG = cdiv(d.W, 32);
  k.Upair = (long long)d.N * d.H * k.SEG; k.U = k.Upair * d.npairs;
#ifdef VMG_DIAG
  { const char* e = getenv("VMG_WGRAD_DBG"); k.dbg = e ? atoi(e) : 0; }
#endif
  const bool b = p.kernel == last_kernel_id(VMG_WGRAD_3B);
  if (b) {
    allow_lds<conv_wgrad3b_kernel>(160 * 1024);
    hipLaunchKernelGGL(conv_wgrad3b_kernel, dim3((unsigned)p.wgs), dim3(W3_THREADS), 6 * W3_BUF, st, k);
  } else {
    allow_lds<conv_wgrad3_kernel>(160 * 1024);
    hipLaunchKernelGGL(conv_wgrad3_kernel, dim3((unsigned)p.wgs), dim3(W3_THREADS), 6 * W3_BUF, st, k);
  }
  VMG_LAUNCH_CHECK();
  hipLaunchKernelGGL(conv_wgrad3_reduce_kernel, dim3(p.rblocks, d.nprob), dim3(256), 0, st, (const float*)d.ws, p.S, p.gx, p.gy, d.Cin, d.Cout, outs, d.I_total, d.o0, d.i0,
                     b ? 1 : 0 /* conv_wgrad3b_kernel keeps the bias sums in the padding tile */);
  VMG_LAUNCH_CHECK();
  return 0;
}

int launch_l2(const WgradCall& d, const WgradPlan& p, hipStream_t st) {
  Lgrad2K k;
  Wgrad3Out outs;
  fill_problems(k, outs, d, p);
  k.Cin = d.Cin; k.Cout = d.Cout;
  k.Mpair = d.M;
  k.Upair = (k.Mpair + 31) / 32; k.U = k.Upair * d.npairs;
  hipLaunchKernelGGL(linear_wgrad2_kernel, dim3((unsigned)p.wgs), dim3(W2_THREADS), 3 * L2_BUF, st, k);
  VMG_LAUNCH_CHECK();
  hipLaunchKernelGGL(linear_wgrad2_reduce_kernel, dim3(p.rblocks, d.nprob), dim3(256), 0, st, (const float*)d.ws, p.S, p.gx, p.gy, d.Cin, d.Cout, outs, d.I_total, d.o0, d.i0);
  VMG_LAUNCH_CHECK();
  return 0;
}

int wgrad_launch(const WgradCall& d, const WgradPlan& p, int facts, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  g_last_kernel = p.kernel;
  const bool bf = d.dtype == VMG_BF16;
  switch (p.kernel) {
    case last_kernel_id(VMG_WGRAD_L2): return launch_l2(d, p, st);
    case last_kernel_id(VMG_WGRAD_3):
    case last_kernel_id(VMG_WGRAD_3B): return launch_w3(d, p, st);
    case last_kernel_id(VMG_WGRAD_7, 1, 3): return launch_w7<1, 3>(d, p, facts, st);
    case last_kernel_id(VMG_WGRAD_7, 1, 7): return launch_w7<1, 7>(d, p, facts, st);
    case last_kernel_id(VMG_WGRAD_7, 2, 7): return launch_w7<2, 7>(d, p, facts, st);
    case last_kernel_id(VMG_WGRAD_7, 4, 7): return launch_w7<4, 7>(d, p, facts, st);
    case last_kernel_id(VMG_WGRAD_V1, 7, 1, 1): return bf ? launch_v1<bf16, 7, 1, 1>(d, p, facts, st) : launch_v1<float, 7, 1, 1>(d, p, facts, st);
    case last_kernel_id(VMG_WGRAD_V1, 3, 1, 4): return launch_v1<bf16, 3, 1, 4>(d, p, facts, st);
    case last_kernel_id(VMG_WGRAD_V1, 3, 1, 1): return launch_v1<bf16, 3, 1, 1>(d, p, facts, st);
    case last_kernel_id(VMG_WGRAD_V1, 3, 3, 1): return bf ? launch_v1<bf16, 3, 3, 1>(d, p, facts, st) : launch_v1<float, 3, 3, 1>(d, p, facts, st);
    case last_kernel_id(VMG_WGRAD_V1, 1, 3, 3): return bf ? launch_v1<bf16, 1, 3, 3>(d, p, facts, st) : launch_v1<float, 1, 3, 3>(d, p, facts, st);
  }
  vmg_set_error("conv_wgrad: no kernel for plan %#x", p.kernel);
  return -1;
}

int g_w3_variant = 1;  // 1: conv_wgrad3b_kernel (buffer-addressed copies between the MFMA columns), 0: conv_wgrad3_kernel

int wgrad_run(const WgradCall& d, void* stream) {
  const int facts = wgrad_pointer_facts(d);
  if (wgrad_validate(d, facts)) return -1;
  const WgradPlan p = wgrad_plan(d, g_w3_variant, facts);
  VMG_CHECK(p.kernel, "conv_wgrad multi: not bf16 operands in aligned 8-channel vectors, too few pixels or too small a workspace for the large-tile kernel (use vmg_conv_wgrad_batched_ws)");
  return wgrad_launch(d, p, facts, stream);
}

}  // namespace

extern "C" int vmg_conv_wgrad_last_kernel(void) { return g_last_kernel; }

extern "C" int vmg_conv_wgrad3_variant(int v) {
  const int prev = g_w3_variant;
  if (v == 0 || v == 1) g_w3_variant = v;
  return prev;
}

extern "C" int64_t vmg_conv_wgrad_ws_bytes(void) { return 320LL * W3_WG_FLOATS * 4; }  // up to 320 workgroups of slabs (~94 MB)

extern "C" int vmg_conv_wgrad_plan(int entry, int dtype, int ks, int nprob, int npairs, int N, int H, int W, int64_t x_ps, int Cin, int64_t dy_ps, int Cout,
                                   int I_total, int o0, int i0, int align, int64_t ws_bytes, int* plan) {
  VMG_CHECK(entry >= VMG_WGRAD_ENTRY_PLAIN && entry <= VMG_WGRAD_ENTRY_MULTI && plan, "conv_wgrad_plan: bad entry or null plan");
  const WgradCall d = {entry, dtype, ks, nprob, npairs, nullptr, nullptr, N, H, W, pixels(N, H, W), x_ps, dy_ps, Cin, Cout, nullptr, nullptr, nullptr, I_total, o0, i0,
                       nullptr, ws_bytes > 0 ? ws_bytes : 0};
  const int facts = align & (VMG_WGRAD_ALIGN_X16 | VMG_WGRAD_ALIGN_DY16 | VMG_WGRAD_ALIGN_DY2);
  if (wgrad_validate(d, facts)) return -1;
  const WgradPlan p = wgrad_plan(d, g_w3_variant, facts);
  const int out[VMG_WGRAD_PLAN_INTS] = {p.kernel, p.gx, p.gy, p.S, (int)p.wgs, p.slabs, p.rblocks};
  memcpy(plan, out, sizeof(out));
  return 0;
}

extern "C" int vmg_conv_wgrad(int dtype, int ks, int N, int H, int W, const void* x, int64_t x_ps, int Cin, const void* dy,
                              int64_t dy_ps, int Cout, float* dW, int I_total, int o0, int i0, float* db, float scale,
                              void* stream) {
  return vmg_conv_wgrad_batched(dtype, ks, 1, &x, &dy, N, H, W, x_ps, Cin, dy_ps, Cout, dW, I_total, o0, i0, db, scale, stream);
}

extern "C" int vmg_conv_wgrad_batched(int dtype, int ks, int npairs, const void* const* x, const void* const* dy, int N, int H, int W,
                                      int64_t x_ps, int Cin, int64_t dy_ps, int Cout, float* dW, int I_total, int o0, int i0,
                                      float* db, float scale, void* stream) {
  const WgradCall d = {VMG_WGRAD_ENTRY_PLAIN, dtype, ks, 1, npairs, x, dy, N, H, W, pixels(N, H, W), x_ps, dy_ps, Cin, Cout, &dW, &db, &scale, I_total, o0, i0,
                       nullptr, 0};
  return wgrad_run(d, stream);
}

extern "C" int vmg_conv_wgrad_batched_ws(int dtype, int ks, int npairs, const void* const* x, const void* const* dy, int N, int H, int W,
                                         int64_t x_ps, int Cin, int64_t dy_ps, int Cout, float* dW, int I_total, int o0, int i0,
                                         float* db, float scale, void* ws, int64_t ws_bytes, void* stream) {
  const WgradCall d = {VMG_WGRAD_ENTRY_WS, dtype, ks, 1, npairs, x, dy, N, H, W, pixels(N, H, W), x_ps, dy_ps, Cin, Cout, &dW, &db, &scale, I_total, o0, i0,
                       ws, ws && ws_bytes > 0 ? ws_bytes : 0};
  return wgrad_run(d, stream);
}

// Several weight gradients of ONE shape (the 30 equal convs of a recurrent residual chain all complete at the same moment of the
// backward pass) in one launch: x / dy hold nprob * npairs pointers [problem][pair], dW / db one pointer per problem.  With one problem per
// launch every conv cuts its pixels into ~85 K slabs to fill the chip and writes 85 x 864 KB of partial sums that a second kernel reads
// back (40 us of a 100 us gradient); with 8 problems per launch a problem needs only ~10 slabs.
extern "C" int vmg_conv_wgrad3_multi(int nprob, int npairs, const void* const* x, const void* const* dy, int N, int H, int W, int64_t x_ps, int Cin,
                                     int64_t dy_ps, int Cout, float* const* dW, int I_total, int o0, int i0, float* const* db, const float* scales,
                                     void* ws, int64_t ws_bytes, void* stream) {
  const WgradCall d = {VMG_WGRAD_ENTRY_MULTI, VMG_BF16, 3, nprob, npairs, x, dy, N, H, W, pixels(N, H, W), x_ps, dy_ps, Cin, Cout, dW, db, scales, I_total, o0, i0,
                       ws, ws_bytes > 0 ? ws_bytes : 0};
  return wgrad_run(d, stream);
}

// Several 1x1 / Linear weight gradients of ONE shape in one launch (the token mixers and projections of a TAB stage): x / dy hold
// nprob * npairs pointers [problem][pair] over M pixels each, dW (O_total, I_total) / db one pointer and scales one factor per problem.
extern "C" int vmg_linear_wgrad2_multi(int nprob, int npairs, const void* const* x, const void* const* dy, int64_t M, int64_t x_ps, int Cin,
                                       int64_t dy_ps, int Cout, float* const* dW, int I_total, int o0, int i0, float* const* db,
                                       const float* scales, void* ws, int64_t ws_bytes, void* stream) {
  const WgradCall d = {VMG_WGRAD_ENTRY_MULTI, VMG_BF16, 1, nprob, npairs, x, dy, 0, 0, 0, M, x_ps, dy_ps, Cin, Cout, dW, db, scales, I_total, o0, i0,
                       ws, ws_bytes > 0 ? ws_bytes : 0};
  return wgrad_run(d, stream);
}
