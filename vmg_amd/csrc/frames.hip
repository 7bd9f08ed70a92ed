// Frame stacks <-> network clips (reference: Tester.evaluate, tools/Tester.py:215-252, with Tester.augment / augment_inverse :387-445):
// uint8 frames as a decoder hands them over become byte / 255 clips, clips become clamp / * 255 / round-half-even uint8 frames, and the
// reference's data_enhance (flip width, flip height, swap the axes, in this order) is folded into the addressing.  One launch, both sides
// described by element strides {frame, channel, row, column}: interleaved, planar, every second frame, crops of larger frames.
//   convert_frames_kernel   a workgroup owns one 32 x 32 tile of one DESTINATION frame, all three channels.  It works out which source rows
//                           and columns the tile shows and fetches them ALONG THE SOURCE ROWS into three byte planes in LDS, then walks the
//                           destination rows and reads plane byte base + r * dr + c * dc, where (dr, dc) is (+-PITCH, +-1) for a straight
//                           and (+-1, +-PITCH) for a transposed tile: the flags choose three scalars, no lane branches on them.
// The planes always hold BYTES: a uint8 source is staged as it is and divided at the store; a float source is clamped, scaled and rounded
// at the load, so the 12 bytes a pixel has in fp32 shrink to 3 before they touch LDS.
// Both global sides move "runs": the elements of one tile row that lie next to each other in memory (planar: 32 elements per channel;
// interleaved: 96 elements, channel fastest).  A run is cut into groups of four elements at the 4-element boundaries of its ADDRESS (16 bytes
// fp32, 8 bf16, 4 uint8); whole groups move as one vector, the partial groups at the two ends element by element.  Nothing outside a run is
// touched, so rows of any byte length and views with any base address are read and written in place; they only have longer scalar tails.
// PITCH = 36 bytes = 9 dwords: a transposed read has the 8 lanes of a destination row 4 plane rows = 36 dwords = 4 banks (mod 32) apart and
// the wave's 8 destination rows within 3 consecutive dwords, so no two lanes of a 32-lane group meet on a bank; straight reads and the
// loads' dword writes walk consecutive dwords.
// The kernel moves bytes; its arithmetic is the correctly rounded byte / 255 and rintf(clamp * 255).  Nothing is added across threads.
#include "common.h"

namespace {

constexpr int TILE = 32;             // destination pixels per tile edge
constexpr int PITCH = TILE + 4;      // bytes per plane row
constexpr int PLANE = TILE * PITCH;  // bytes per channel plane
constexpr int THREADS = 256;

enum { LAY_GENERIC = 0, LAY_PLANAR = 1, LAY_INTER = 2 };

struct FrameSide {
  long long sf, sc, sr, sp;  // element strides: frame, channel, row, column
  int layout;
};

struct ConvertArgs {
  const void* src;
  void* dst;
  FrameSide s, d;
  int H, W;    // source frame
  int dh, dw;  // destination frame: (W, H) when rot
  int tx, ty, hf, vf, rot;
};

// ---- one element in, one byte out ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned int to_byte(float x) {
  // tools/Tester.py:249-250: clamp(0, 1), * 255.0 in float32, numpy's round (half to even) = rintf in the default rounding mode
  return (unsigned int)rintf(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f);
}
__device__ __forceinline__ unsigned int load_byte(const unsigned char* p) { return *p; }
__device__ __forceinline__ unsigned int load_byte(const float* p) { return to_byte(*p); }
__device__ __forceinline__ unsigned int load_byte(const bf16* p) { return to_byte((float)*p); }

// four elements at a 4-element boundary -> four bytes, first element lowest
__device__ __forceinline__ unsigned int load_bytes4(const unsigned char* p) { return *reinterpret_cast<const unsigned int*>(p); }
__device__ __forceinline__ unsigned int load_bytes4(const float* p) {
  float v[4];
  load4(p, v);
  return to_byte(v[0]) | to_byte(v[1]) << 8 | to_byte(v[2]) << 16 | to_byte(v[3]) << 24;
}
__device__ __forceinline__ unsigned int load_bytes4(const bf16* p) {
  float v[4];
  load4(p, v);
  return to_byte(v[0]) | to_byte(v[1]) << 8 | to_byte(v[2]) << 16 | to_byte(v[3]) << 24;
}

// ---- one byte in, one element out ---------------------------------------------------------------------------------------------------
// numpy's astype(np.float32) / 255. is the correctly rounded fp32 quotient: the intrinsic, not a bare `/` (which may become a reciprocal)
__device__ __forceinline__ float unit(unsigned int b) { return __fdiv_rn((float)b, 255.0f); }
__device__ __forceinline__ void store_byte(unsigned char* p, unsigned int b) { *p = (unsigned char)b; }
__device__ __forceinline__ void store_byte(float* p, unsigned int b) { *p = unit(b); }
__device__ __forceinline__ void store_byte(bf16* p, unsigned int b) { *p = (bf16)unit(b); }

__device__ __forceinline__ void store_bytes4(unsigned char* p, const unsigned int b[4]) {
  *reinterpret_cast<unsigned int*>(p) = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
}
__device__ __forceinline__ void store_bytes4(float* p, const unsigned int b[4]) {
  const float v[4] = {unit(b[0]), unit(b[1]), unit(b[2]), unit(b[3])};
  store4(p, v);
}
__device__ __forceinline__ void store_bytes4(bf16* p, const unsigned int b[4]) {
  const float v[4] = {unit(b[0]), unit(b[1]), unit(b[2]), unit(b[3])};
  store4(p, v);
}

// groups of four that cover a run of n elements from any start: at most 3 elements in front of the run and 3 behind it
__host__ __device__ constexpr int groups_for(int n) { return (n + 3 + 3) / 4; }

template <typename TS, typename TD>
__global__ __launch_bounds__(THREADS) void convert_frames_kernel(ConvertArgs a) {
  __shared__ __attribute__((aligned(4))) unsigned char tile[3 * PLANE];
  const int tid = threadIdx.x;

  // workgroup-uniform: which frame, which tile of it, the source window it shows
  const int per = a.tx * a.ty;
  const int f = blockIdx.x / per, t = blockIdx.x - f * per;
  const int R0 = (t / a.tx) * TILE, C0 = (t - (t / a.tx) * a.tx) * TILE;  // the tile's first destination row / column
  const int th = min(TILE, a.dh - R0), tw = min(TILE, a.dw - C0);
  // destination (r, c) shows source (vf ? H - 1 - i : i, hf ? W - 1 - j : j) with (i, j) = rot ? (c, r) : (r, c)
  const int i0 = a.rot ? C0 : R0, ni = a.rot ? tw : th, j0 = a.rot ? R0 : C0, nj = a.rot ? th : tw;
  const int sy0 = a.vf ? a.H - i0 - ni : i0, sx0 = a.hf ? a.W - j0 - nj : j0;  // source rows sy0 .. sy0 + ni, columns sx0 .. sx0 + nj, ascending

  // ---- source -> planes: plane byte (channel k, row r, column x) = source (sy0 + r, sx0 + x) of channel k --------------------------------
  const TS* sbase = static_cast<const TS*>(a.src) + (long long)f * a.s.sf + (long long)sy0 * a.s.sr + (long long)sx0 * a.s.sp;
  if (a.s.layout == LAY_GENERIC) {
    const bool ch_fast = a.s.sc < a.s.sp;  // consecutive lanes follow the source's fastest axis
    for (int i = tid; i < ni * nj * 3; i += THREADS) {
      const int r = i / (3 * nj), k = i - r * 3 * nj;
      const int c = ch_fast ? k % 3 : k / nj, x = ch_fast ? k / 3 : k % nj;
      tile[c * PLANE + r * PITCH + x] = (unsigned char)load_byte(sbase + c * a.s.sc + (long long)r * a.s.sr + (long long)x * a.s.sp);
    }
  } else {
    const bool inter = a.s.layout == LAY_INTER;
    const int runs = inter ? 1 : 3, n = inter ? 3 * nj : nj;  // runs per source row, elements per run
    const int G = inter ? groups_for(3 * TILE) : groups_for(TILE);
    for (int i = tid; i < ni * runs * G; i += THREADS) {
      const int g = i % G, q = (i / G) % runs, r = i / (G * runs);
      const TS* run = sbase + (long long)r * a.s.sr + (inter ? 0 : q * a.s.sc);
      const int lead = (int)(((uintptr_t)run / sizeof(TS)) & 3);  // elements between the 4-element boundary below the run and its start
      const int e0 = 4 * g - lead;
      if (e0 >= n || e0 + 4 <= 0) continue;
      unsigned int word = 0;
      if (e0 >= 0 && e0 + 4 <= n) {
        word = load_bytes4(run + e0);
        if (!inter && lead == 0) {  // four pixels of one channel at a dword of the plane
          *reinterpret_cast<unsigned int*>(tile + q * PLANE + r * PITCH + e0) = word;
          continue;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (e0 + k >= 0 && e0 + k < n) word |= load_byte(run + e0 + k) << (8 * k);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = e0 + k;
        if (e < 0 || e >= n) continue;
        const int px = inter ? (int)((unsigned int)e / 3u) : e, c = inter ? e - 3 * px : q;
        tile[c * PLANE + r * PITCH + px] = (unsigned char)(word >> (8 * k));
      }
    }
  }
  __syncthreads();

  // ---- planes -> destination ------------------------------------------------------------------------------------------------------------
  const int dy = a.vf ? -PITCH : PITCH, dx = a.hf ? -1 : 1;
  const int origin = (a.vf ? (ni - 1) * PITCH : 0) + (a.hf ? nj - 1 : 0);
  const int dr = a.rot ? dx : dy, dc = a.rot ? dy : dx;
  TD* dbase = static_cast<TD*>(a.dst) + (long long)f * a.d.sf + (long long)R0 * a.d.sr + (long long)C0 * a.d.sp;
  if (a.d.layout == LAY_GENERIC) {
    const bool ch_fast = a.d.sc < a.d.sp;
    for (int i = tid; i < th * tw * 3; i += THREADS) {
      const int r = i / (3 * tw), k = i - r * 3 * tw;
      const int c = ch_fast ? k % 3 : k / tw, x = ch_fast ? k / 3 : k % tw;
      store_byte(dbase + c * a.d.sc + (long long)r * a.d.sr + (long long)x * a.d.sp, tile[c * PLANE + origin + r * dr + x * dc]);
    }
    return;
  }
  const bool inter = a.d.layout == LAY_INTER;
  const int runs = inter ? 1 : 3, n = inter ? 3 * tw : tw;
  const int G = inter ? groups_for(3 * TILE) : groups_for(TILE);
  for (int i = tid; i < th * runs * G; i += THREADS) {
    // planar: the three channels of a row are the slowest index, so that a wave's lanes read one plane
    const int g = i % G, r = (i / G) % th, q = i / (G * th);
    TD* run = dbase + (long long)r * a.d.sr + (inter ? 0 : q * a.d.sc);
    const int lead = (int)(((uintptr_t)run / sizeof(TD)) & 3);
    const int e0 = 4 * g - lead;
    if (e0 >= n || e0 + 4 <= 0) continue;
    unsigned int b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = min(max(e0 + k, 0), n - 1);  // (clamped: an element outside the run is read, never stored)
      const int px = inter ? (int)((unsigned int)e / 3u) : e, c = inter ? e - 3 * px : q;
      b[k] = tile[c * PLANE + origin + r * dr + px * dc];
    }
    if (e0 >= 0 && e0 + 4 <= n) {
      store_bytes4(run + e0, b);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e0 + k >= 0 && e0 + k < n) store_byte(run + e0 + k, b[k]);
    }
  }
}

int elem_size(int type) { return type == VMG_FRAME_U8 ? 1 : type == VMG_FRAME_BF16 ? 2 : 4; }

int layout_of(const FrameSide& s) {
  if (s.sp == 1) return LAY_PLANAR;
  if (s.sp == 3 && s.sc == 1) return LAY_INTER;
  return LAY_GENERIC;
}

// the last element a side reaches, in elements from its base
long long reach(const FrameSide& s, int T, int h, int w) { return (T - 1) * s.sf + 2 * s.sc + (h - 1) * s.sr + (w - 1) * s.sp; }

// no two index tuples of a side may name one element: sorted by stride, every axis must step over all that the smaller ones span
bool injective(const FrameSide& s, int T, int h, int w) {
  long long st[4] = {s.sf, s.sc, s.sr, s.sp};
  long long ex[4] = {T, 3, h, w};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (st[j] < st[i]) {
        const long long a = st[i], b = ex[i];
        st[i] = st[j], ex[i] = ex[j], st[j] = a, ex[j] = b;
      }
  long long span = 0;  // the largest offset the axes so far reach
  for (int i = 0; i < 4; ++i) {
    if (ex[i] == 1) continue;
    if (st[i] <= span) return false;
    span += (ex[i] - 1) * st[i];
  }
  return true;
}

}  // namespace

extern "C" int vmg_convert_frames(int src_type, const void* src, const int64_t* src_strides, int dst_type, void* dst, const int64_t* dst_strides, int T,
                                  int H, int W, int flags, void* stream) {
  VMG_CHECK(src && dst && src_strides && dst_strides, "convert_frames: null argument");
  VMG_CHECK(T >= 1 && T <= (1 << 20) && H >= 1 && W >= 1 && H <= (1 << 16) && W <= (1 << 16), "convert_frames: %d frames of %d x %d out of range", T, H, W);
  VMG_CHECK(flags >= 0 && flags < 8, "convert_frames: flags are hflip | vflip << 1 | rot90 << 2, got %d", flags);
  const bool s_ok = src_type == VMG_FRAME_U8 || src_type == VMG_FRAME_F32 || src_type == VMG_FRAME_BF16;
  const bool d_ok = dst_type == VMG_FRAME_U8 || dst_type == VMG_FRAME_F32 || dst_type == VMG_FRAME_BF16;
  VMG_CHECK(s_ok && d_ok && (src_type == VMG_FRAME_U8 || dst_type == VMG_FRAME_U8),
            "convert_frames: uint8 -> fp32 / bf16 / uint8 and fp32 / bf16 -> uint8 are the type pairs, got %d -> %d", src_type, dst_type);
  ConvertArgs a;
  a.src = src, a.dst = dst;
  a.s.sf = src_strides[0], a.s.sc = src_strides[1], a.s.sr = src_strides[2], a.s.sp = src_strides[3];
  a.d.sf = dst_strides[0], a.d.sc = dst_strides[1], a.d.sr = dst_strides[2], a.d.sp = dst_strides[3];
  a.H = H, a.W = W;
  a.hf = flags & 1, a.vf = (flags >> 1) & 1, a.rot = (flags >> 2) & 1;
  a.dh = a.rot ? W : H, a.dw = a.rot ? H : W;
  for (int i = 0; i < 4; ++i) {
    VMG_CHECK(src_strides[i] >= 0 && dst_strides[i] >= 0, "convert_frames: negative stride");
    VMG_CHECK(src_strides[i] < (1LL << 40) && dst_strides[i] < (1LL << 40), "convert_frames: stride out of range");
  }
  VMG_CHECK(injective(a.d, T, a.dh, a.dw), "convert_frames: the destination's strides {%lld, %lld, %lld, %lld} make %d x 3 x %d x %d elements overlap",
            (long long)a.d.sf, (long long)a.d.sc, (long long)a.d.sr, (long long)a.d.sp, T, a.dh, a.dw);
  const int ss = elem_size(src_type), ds = elem_size(dst_type);
  VMG_CHECK(((uintptr_t)src % ss) == 0 && ((uintptr_t)dst % ds) == 0, "convert_frames: a pointer is not aligned to its element");
  const uintptr_t s_lo = (uintptr_t)src, s_hi = s_lo + (uintptr_t)(reach(a.s, T, H, W) + 1) * ss;
  const uintptr_t d_lo = (uintptr_t)dst, d_hi = d_lo + (uintptr_t)(reach(a.d, T, a.dh, a.dw) + 1) * ds;
  VMG_CHECK(s_hi <= d_lo || d_hi <= s_lo, "convert_frames: source and destination overlap (the conversion does not run in place)");
  a.s.layout = layout_of(a.s), a.d.layout = layout_of(a.d);
  a.tx = cdiv(a.dw, TILE), a.ty = cdiv(a.dh, TILE);
  const int64_t tiles = (int64_t)T * a.tx * a.ty;
  VMG_CHECK(tiles < (1LL << 31), "convert_frames: %lld tiles in one call, at most 2^31 - 1", (long long)tiles);

  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned int)tiles), block(THREADS);
#define VMG_CONVERT(TS, TD) hipLaunchKernelGGL((convert_frames_kernel<TS, TD>), grid, block, 0, st, a)
  if (src_type == VMG_FRAME_U8) {
    if (dst_type == VMG_FRAME_U8) VMG_CONVERT(unsigned char, unsigned char);
    else if (dst_type == VMG_FRAME_F32) VMG_CONVERT(unsigned char, float);
    else VMG_CONVERT(unsigned char, bf16);
  } else if (src_type == VMG_FRAME_F32) {
    VMG_CONVERT(float, unsigned char);
  } else {
    VMG_CONVERT(bf16, unsigned char);
  }
#undef VMG_CONVERT
  VMG_LAUNCH_CHECK();
  return 0;
}
