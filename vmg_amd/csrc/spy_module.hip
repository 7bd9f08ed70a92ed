// One SPyNet basic module (models/vmg.py:126-173: five 7x7 convolutions 8 -> 32 -> 64 -> 32 -> 16 -> 2, ReLU after the first four) on a
// coarse pyramid level as ONE launch per direction: vmg_spy_module_fwd / vmg_spy_module_bwd (bf16, h * w <= 256, one workgroup per image).
//
// At 2 x 2 .. 16 x 16 pixels a 7x7 convolution launch of conv_igemm_kernel<bf16, 7, 1, NTB> is 48 - 192 workgroups that each walk a
// serial loop of 7 - 14 stages: 8 - 12 us for a few MFLOP, ten launches per level and step.  Here the level's image stays in LDS: the
// activations ping-pong between two tiles with a 3-pixel zero border, the packed weights stream through a 2-slot LDS ring straight from
// the packs the per-conv route reads (vmg_conv_pack, same cout_tiles), and every intermediate the weight gradients need still goes to
// global memory.
//
// SAME BITS as the per-conv route, per output element: the same k-steps (32-channel block, tap row ky, tap kx; lane group g holds chunk
// 4 * cbk + g, padding chunks read the last real chunk against zero weights) feed the same v_mfma_f32_16x16x32_bf16 in the same order
// from a zero accumulator; bias is added to the fp32 sum, ReLU is `v > 0 ? v : v * 0`, the ReLU derivative of the backward multiplies
// the fp32 value, and the one bf16 rounding is that of the store -- the next convolution reads those bf16 values (from LDS here, from
// global memory there).  Which 16 pixels share an MFMA does not enter a pixel's sum, so the pixels are taken in groups of 16 of the
// flattened image (wave w owns groups w * MT .. w * MT + MT - 1).
//
// Measured (profiles/r06_a_spynet_ab.txt): 34 us per launch at 2 x 2 .. 8 x 8, 81 us at 16 x 16 -- 660 KB of packed weights per workgroup at
// about 19 GB/s, the rate of one ring slot in flight behind `s_waitcnt vmcnt(0)` (the per-conv kernel streams at the same rate).  Reading the
// fragments of a whole tap row ahead of its MFMAs changed neither figure: the ring, not the LDS latency, is what a next version deepens.
// On levels of <= 16 pixels waves 1..3 hold no pixel and compute pixel 0 for nothing; letting them skip the k loop (barriers and ring fills
// kept), and fetching the backward's ReLU-derivative operands in one batch ahead of the epilogue's stores (clamped addresses), were
// measured together and the second alone: the small-level launches went from 6 x 34 us to 6 x 78 us both times, cause not found, so neither is in.
#include "common.h"

namespace {

// geometry of a 7x7 bf16 pack (conv_igemm.hip: kstg, stage_bytes, stage_stride, stages_of)
constexpr int KS = 7, RAD = 3, CB = 16;
constexpr int spy_stage_stride(int ntb) { return (KS * 4 * ntb * 16 * CB + 4095) / 4096 * 4096; }
inline int spy_stages(int ch) { return KS * ((ch / 8 + 3) / 4); }

constexpr int NLAYER = 5;

struct SpyLayer {
  const char* pack;   // [stage][k-step j][lane group g][co][8] bf16, stage stride ss
  const float* bias;  // null: none
  const bf16* aux;    // null, or (N, h, w, cout): the output is multiplied by aux > 0 ? 1 : 0
  bf16* out;          // null, or (N, h, w, cout)
  int cin, cout, ntb, relu;
  int nst;   // stages (32-channel block x tap row)
  int grp;   // stages per ring slot
  int ss;    // stage stride, bytes
  int pixb;  // LDS pixel stride of this layer's INPUT tile, bytes
};

struct SpyK {
  SpyLayer L[NLAYER];
  const bf16* x;  // (N, h, w, 8)
  int nl, H, W;
  int buf_off[2];  // LDS offsets of the two activation tiles (layer l reads tile l & 1)
  int buf_bytes[2];
  int ring_off, slot;  // weight ring: 2 slots of `slot` bytes
};

// LDS-DMA, 16 bytes per lane to lds_dst + 16 * lane (wave-uniform lds_dst); see conv_igemm.hip::glds16_asm.  hipcc does not drain it at a
// barrier: the consumer waits s_waitcnt vmcnt(0) first.
__device__ __forceinline__ void spy_glds16(const char* gsrc, char* lds_dst) {
  unsigned keep;
  const unsigned ldst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)LDS_PTR(lds_dst));
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(ldst) : "memory");
}

// ring slot piece `piece` of layer L (grp stages = up to `slot` bytes) -> ring slot `s`: wave w issues the 1-KiB pieces w, w + 4, ...
__device__ __forceinline__ void spy_issue(const SpyK& a, const SpyLayer& L, int piece, int s, char* smem, int wave, int lane) {
  const int st0 = piece * L.grp;
  const int nstg = min(L.grp, L.nst - st0);
  const int kib = nstg * (L.ss >> 10);
  const char* g = L.pack + (long long)st0 * L.ss + lane * 16;
  char* d = smem + a.ring_off + s * a.slot;
  for (int i = wave; i < kib; i += 4) spy_glds16(g + i * 1024, d + i * 1024);
}

template <int MT, int NTB>
__device__ __forceinline__ void spy_layer(const SpyK& a, int l, int& gpiece, char* smem, int n) {
  const SpyLayer& L = a.L[l];
  constexpr int COB = NTB * 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int px = lane & 15, g = lane >> 4;
  const int H = a.H, W = a.W, hw = H * W, TW = W + 2 * RAD;
  const int pixb = L.pixb, CH = L.cin >> 3;
  const char* in = smem + a.buf_off[l & 1];
  const bool last = l + 1 >= a.nl;

  // the next layer's input tile: zeros (its border stays zero; the epilogue below writes the image)
  if (!last) {
    char* dst = smem + a.buf_off[(l + 1) & 1];
    const int nb = a.buf_bytes[(l + 1) & 1];
    for (int i = tid * 16; i < nb; i += 256 * 16) *reinterpret_cast<uint4*>(dst + i) = make_uint4(0, 0, 0, 0);
  }

  f32x4 acc[NTB][MT];
#pragma unroll
  for (int ct = 0; ct < NTB; ++ct)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[ct][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // per-lane pixel base addresses in the input tile (lanes past the image compute pixel 0 and store nothing)
  const char* pixp[MT];
  int pidx[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int p = (wave * MT + mt) * 16 + px;
    pidx[mt] = p;
    const int pc = p < hw ? p : 0;
    const int y = pc / W, x = pc - y * W;
    pixp[mt] = in + (y * TW + x) * pixb;
  }

  const int npiece = (L.nst + L.grp - 1) / L.grp;
  int sl = 0;
  for (int pc = 0; pc < npiece; ++pc, ++gpiece) {
    // piece gpiece has landed, and every wave is past piece gpiece - 1 before its slot is refilled
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (pc + 1 < npiece) spy_issue(a, L, pc + 1, (gpiece + 1) & 1, smem, wave, lane);
    else if (!last) spy_issue(a, a.L[l + 1], 0, (gpiece + 1) & 1, smem, wave, lane);
    const char* slot = smem + a.ring_off + (gpiece & 1) * a.slot + g * (COB * CB) + px * CB;
    const int nstg = min(L.grp, L.nst - pc * L.grp);
    for (int s = 0; s < nstg; ++s, ++sl) {
      const int cbk = sl / KS, ky = sl - cbk * KS;
      const int base = ky * (TW * pixb) + min(4 * cbk + g, CH - 1) * CB;
      const char* wslot = slot + s * L.ss;
      bf16x8 xf[2][MT], wf[2][NTB];
      auto load_frags = [&](int j, int set) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) xf[set][mt] = *reinterpret_cast<const bf16x8*>(pixp[mt] + base + j * pixb);
#pragma unroll
        for (int ct = 0; ct < NTB; ++ct) wf[set][ct] = *reinterpret_cast<const bf16x8*>(wslot + j * (4 * COB * CB) + ct * 16 * CB);
      };
      load_frags(0, 0);
#pragma unroll
      for (int j = 0; j < KS; ++j) {
        if (j + 1 < KS) load_frags(j + 1, (j + 1) & 1);
#pragma unroll
        for (int ct = 0; ct < NTB; ++ct)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[ct][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j & 1][ct], xf[j & 1][mt], acc[ct][mt], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: a lane holds output channels ct * 16 + 4 g .. + 3 of pixel px of each of its groups
  const int cout = L.cout;
  char* nxt = last ? nullptr : smem + a.buf_off[(l + 1) & 1];
  const int npixb = last ? 0 : a.L[l + 1].pixb;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int p = pidx[mt];
    if (p >= hw) continue;
    const long long pix = (long long)n * hw + p;
    const int y = p / W, x = p - y * W;
#pragma unroll
    for (int ct = 0; ct < NTB; ++ct) {
      const int co0 = ct * 16 + g * 4;
      if (co0 >= cout) continue;
      float v[4] = {acc[ct][mt][0], acc[ct][mt][1], acc[ct][mt][2], acc[ct][mt][3]};
      if (co0 + 4 <= cout) {
        if (L.bias) {
          const float4 bv = *reinterpret_cast<const float4*>(L.bias + co0);
          v[0] += bv.x; v[1] += bv.y; v[2] += bv.z; v[3] += bv.w;
        }
        if (L.relu) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = v[r] > 0.f ? v[r] : v[r] * 0.f;
        }
        if (L.aux) {
          float u[4];
          load4(L.aux + pix * cout + co0, u);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] *= u[r] > 0.f ? 1.f : 0.f;
        }
        const bf16x4 t = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
        if (L.out) *reinterpret_cast<bf16x4*>(L.out + pix * cout + co0) = t;
        if (nxt) *reinterpret_cast<bf16x4*>(nxt + ((y + RAD) * TW + x + RAD) * npixb + co0 * 2) = t;
      } else {
        // fewer than 4 channels left (the flow residual: 2): element-wise; always a last layer
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (co0 + r < cout) {
            float t = v[r];
            if (L.bias) t += L.bias[co0 + r];
            if (L.relu) t = t > 0.f ? t : t * 0.f;
            if (L.out) L.out[pix * cout + co0 + r] = (bf16)t;
          }
        }
      }
    }
  }
  __syncthreads();  // the next layer's tile is written; this layer's tile is free
}

template <int MT>
__global__ __launch_bounds__(256) void spy_module_kernel(const SpyK a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x;
  const int H = a.H, W = a.W, hw = H * W, TW = W + 2 * RAD;

  spy_issue(a, a.L[0], 0, 0, smem, wave, lane);
  {
    // the 8-channel operand tile: zeros, then the image (one 16-byte pixel per thread; every lane loads, lanes past the image pixel 0)
    char* t0 = smem + a.buf_off[0];
    for (int i = tid * 16; i < a.buf_bytes[0]; i += 256 * 16) *reinterpret_cast<uint4*>(t0 + i) = make_uint4(0, 0, 0, 0);
    const int pc = tid < hw ? tid : 0;
    const uint4 v = *reinterpret_cast<const uint4*>(a.x + ((long long)n * hw + pc) * 8);
    __syncthreads();
    const int y = pc / W, x = pc - y * W;
    if (tid < hw) *reinterpret_cast<uint4*>(t0 + ((y + RAD) * TW + x + RAD) * a.L[0].pixb) = v;
  }
  int gpiece = 0;
  for (int l = 0; l < a.nl; ++l) {
    switch (a.L[l].ntb) {
      case 1: spy_layer<MT, 1>(a, l, gpiece, smem, n); break;
      case 2: spy_layer<MT, 2>(a, l, gpiece, smem, n); break;
      default: spy_layer<MT, 4>(a, l, gpiece, smem, n); break;
    }
  }
}

constexpr int SPY_LDS = 160 * 1024;

template <int MT>
int spy_launch_mt(const SpyK& k, int N, int lds, hipStream_t st) {
  auto fn = spy_module_kernel<MT>;
  static bool attr_set[VMG_MAX_DEVICES] = {};
  const int dev = vmg_current_device();
  if (!attr_set[dev]) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, SPY_LDS);
    attr_set[dev] = true;
  }
  hipLaunchKernelGGL(fn, dim3((unsigned)N), dim3(256), lds, st, k);
  VMG_LAUNCH_CHECK();
  return 0;
}

// tiles per workgroup of the per-conv route's packs (kernels.cout_tiles_for, ks = 7)
int spy_tiles(int cout) {
  const int t = (cout + 15) / 16;
  return t <= 1 ? 1 : (t == 2 ? 2 : 4);
}

// lays the layers out in LDS and launches; k.L[i].{pack, bias, aux, out, cin, cout, relu} and k.x / nl / H / W are filled in
int spy_launch(SpyK& k, int N, hipStream_t st) {
  const int H = k.H, W = k.W, hw = H * W;
  const int tile_px = (H + 2 * RAD) * (W + 2 * RAD);
  int max_ss = 0;
  for (int l = 0; l < k.nl; ++l) {
    SpyLayer& L = k.L[l];
    VMG_CHECK(L.cin % 8 == 0 && L.cin >= 8 && L.cin <= 64 && L.cout >= 1 && L.cout <= 64, "spy_module: layer %d: %d -> %d channels", l, L.cin, L.cout);
    VMG_CHECK(l + 1 >= k.nl || (L.cout % 8 == 0 && L.cout == k.L[l + 1].cin), "spy_module: layer %d feeds %d channels into %d", l, L.cout, k.L[l + 1].cin);
    VMG_CHECK(L.pack && ((uintptr_t)L.pack & 15) == 0, "spy_module: layer %d: null / unaligned pack", l);
    VMG_CHECK(!L.aux || L.cout % 4 == 0, "spy_module: layer %d: a ReLU-derivative operand needs cout %% 4 == 0 (got %d)", l, L.cout);
    L.ntb = spy_tiles(L.cout);
    L.ss = spy_stage_stride(L.ntb);
    L.nst = spy_stages(L.cin);
    if (L.ss > max_ss) max_ss = L.ss;
  }
  // input tiles: a padded pixel stride (no 2^n stride between the 16 pixels of a fragment read) where LDS has the room
  int lds = 0;
  for (int pad = 2; pad >= 0; --pad) {  // 2: every 32- / 64-channel tile padded; 1: the 32-channel tiles only; 0: dense
    int need[2] = {0, 0};
    for (int l = 0; l < k.nl; ++l) {
      SpyLayer& L = k.L[l];
      const bool p = (L.cin % 32 == 0) && (pad == 2 || (pad == 1 && L.cin == 32));
      L.pixb = L.cin * 2 + (p ? 16 : 0);
      const int b = tile_px * L.pixb;
      if (b > need[l & 1]) need[l & 1] = b;
    }
    k.buf_bytes[0] = need[0]; k.buf_bytes[1] = need[1];
    k.buf_off[0] = 0; k.buf_off[1] = (need[0] + 1023) & ~1023;
    k.ring_off = k.buf_off[1] + ((need[1] + 1023) & ~1023);
    k.slot = ((SPY_LDS - k.ring_off) / 2) & ~4095;
    if (k.slot >= max_ss) break;
    VMG_CHECK(pad > 0, "spy_module: a %d x %d level does not fit LDS", H, W);
  }
  if (k.slot > 64 * 1024) k.slot = 64 * 1024;
  for (int l = 0; l < k.nl; ++l) {
    SpyLayer& L = k.L[l];
    L.grp = k.slot / L.ss;
    if (L.grp > L.nst) L.grp = L.nst;
  }
  lds = k.ring_off + 2 * k.slot;
  VMG_CHECK(lds <= SPY_LDS, "spy_module: LDS request %d B", lds);
  const int groups = (hw + 15) / 16, mt = (groups + 3) / 4;
  if (mt == 1) return spy_launch_mt<1>(k, N, lds, st);
  if (mt == 2) return spy_launch_mt<2>(k, N, lds, st);
  return spy_launch_mt<4>(k, N, lds, st);
}

int spy_check(const vmg_spy_module_desc* d, const char* who) {
  VMG_CHECK(d != nullptr, "%s: null descriptor", who);
  VMG_CHECK(d->N > 0 && d->H > 0 && d->W > 0 && d->H * d->W <= 256 && (d->H + 2 * RAD) * (d->W + 2 * RAD) <= 484, "%s: %d images of %d x %d (h * w <= 256, (h + 6)(w + 6) <= 484)", who,
            d->N, d->H, d->W);
  VMG_CHECK(d->x && ((uintptr_t)d->x & 15) == 0, "%s: null / unaligned operand", who);
  for (int i = 0; i < 5; ++i) VMG_CHECK(d->packed[i], "%s: null pack %d", who, i);
  return 0;
}

constexpr int SPY_CH[6] = {8, 32, 64, 32, 16, 2};

}  // namespace

extern "C" int vmg_spy_module_fwd(const vmg_spy_module_desc* d, void* stream) {
  if (spy_check(d, "spy_module_fwd")) return -1;
  VMG_CHECK(d->out, "spy_module_fwd: null output");
  const bool keep = d->y[0] != nullptr;
  SpyK k;
  memset(&k, 0, sizeof(k));
  k.x = (const bf16*)d->x; k.nl = 5; k.H = d->H; k.W = d->W;
  for (int i = 0; i < 5; ++i) {
    SpyLayer& L = k.L[i];
    VMG_CHECK(d->bias[i], "spy_module_fwd: null bias %d", i);
    VMG_CHECK(i == 4 || (d->y[i] != nullptr) == keep, "spy_module_fwd: y0..y3 are all given or all null");
    VMG_CHECK(i == 4 || ((uintptr_t)d->y[i] & 7) == 0, "spy_module_fwd: unaligned y%d", i);
    L.pack = (const char*)d->packed[i]; L.bias = d->bias[i]; L.cin = SPY_CH[i]; L.cout = SPY_CH[i + 1]; L.relu = i < 4;
    L.out = (bf16*)(i < 4 ? d->y[i] : d->out);
  }
  return spy_launch(k, d->N, (hipStream_t)stream);
}

extern "C" int vmg_spy_module_bwd(const vmg_spy_module_desc* d, void* stream) {
  if (spy_check(d, "spy_module_bwd")) return -1;
  SpyK k;
  memset(&k, 0, sizeof(k));
  k.x = (const bf16*)d->x; k.nl = d->out ? 5 : 4; k.H = d->H; k.W = d->W;
  VMG_CHECK(!d->out || ((uintptr_t)d->out & 7) == 0, "spy_module_bwd: unaligned dx");
  for (int l = 0; l < k.nl; ++l) {  // layer l = the data gradient of conv (4 - l): dpre_(4-l) (padded to 8 channels for the last conv) -> dpre_(3-l) / dx
    SpyLayer& L = k.L[l];
    const int c = 4 - l;
    L.pack = (const char*)d->packed[c];
    L.cin = c == 4 ? 8 : SPY_CH[c + 1];
    L.cout = SPY_CH[c];
    if (c > 0) {
      VMG_CHECK(d->y[c - 1] && d->dpre[c - 1] && (((uintptr_t)d->y[c - 1] | (uintptr_t)d->dpre[c - 1]) & 7) == 0, "spy_module_bwd: null / unaligned y%d / dpre%d", c - 1, c - 1);
      L.aux = (const bf16*)d->y[c - 1];
      L.out = (bf16*)d->dpre[c - 1];
    } else {
      L.out = (bf16*)d->out;
    }
  }
  return spy_launch(k, d->N, (hipStream_t)stream);
}
