// Training batches from resident frames (reference: data/REDS.py:188-215, data/Vimeo.py:179-206): N crops, each out of its own uint8
// frame, flipped / transposed per crop, channels reordered, written as one contiguous planar (N, 3, ch, cw) tensor, one launch.
//   crop_batch_kernel   a workgroup owns one 32 x 32 tile of one crop's output, all three channels.  It reads the crop's descriptor and
//                       frame pointer once (workgroup-uniform: scalar registers), works out which rows and columns of the SOURCE the tile
//                       shows, and fetches them along the source rows into three byte planes in LDS, whatever the flags: dwords where
//                       the rows of the store start 4-byte-congruent (the run begins up to 3 bytes early), bytes for dwords that would
//                       leave the frame's row and for stores of any other strides.  The planes are the transpose buffer: the store
//                       walks the output rows, 4 pixels per thread and channel as one 16 / 8 / 4-byte store, and reads plane byte
//                       base + r * dr + c * dc, where (dr, dc) is (+-PITCH, +-1) for a straight and (+-1, +-PITCH) for a transposed crop:
//                       the flags only choose three scalars, no lane branches on them.
// PITCH = 36 bytes = 9 dwords: a transposed read has the 8 lanes of an output row 4 plane rows = 36 dwords = 4 banks (mod 32) apart and
// the wave's 8 output rows within 3 consecutive dwords: no two lanes of a 32-lane group share a bank.
// The kernel moves bytes; its only arithmetic is the correctly rounded byte / 255.  Nothing is added across threads: same input, same bits.
#include "common.h"

namespace {

constexpr int TILE = 32;            // output pixels per tile edge
constexpr int PITCH = TILE + 4;     // bytes per plane row
constexpr int PLANE = TILE * PITCH; // bytes per channel plane
constexpr int IDW = (3 * TILE + 3 + 3) / 4;  // dwords that cover 96 interleaved bytes from any misaligned start
constexpr int PDW = (TILE + 3 + 3) / 4;      // the same for 32 planar bytes

enum { CB_BYTES = 0, CB_PLANAR_DWORDS = 1, CB_INTER_DWORDS = 2 };

struct CropArgs {
  const unsigned char* const* frames;  // N frame base addresses (device)
  const int* desc;                     // N x {y0, x0, flags} (device)
  long long sr, sp, sc;                // byte strides: row, pixel, channel
  int H, W, ch, cw, tx, ty, crev, mode, out_type;
  void* out;
};

__device__ __forceinline__ void store1(void* out, int out_type, long long idx, unsigned int b) {
  if (out_type == VMG_CROP_U8) {
    static_cast<unsigned char*>(out)[idx] = (unsigned char)b;
    return;
  }
  const float x = __fdiv_rn((float)b, 255.0f);  // the correctly rounded quotient, as numpy's astype(float32) / 255.
  if (out_type == VMG_CROP_F32)
    static_cast<float*>(out)[idx] = x;
  else
    static_cast<bf16*>(out)[idx] = (bf16)x;
}

__global__ __launch_bounds__(256) void crop_batch_kernel(CropArgs a) {
  __shared__ __attribute__((aligned(4))) unsigned char tile[3 * PLANE];
  const int tid = threadIdx.x;

  // workgroup-uniform: which crop, which tile of it, its descriptor
  const int per = a.tx * a.ty;
  const int n = blockIdx.x / per, t = blockIdx.x - n * per;
  const int R0 = (t / a.tx) * TILE, C0 = (t - (t / a.tx) * a.tx) * TILE;  // the tile's first output row / column
  const int th = min(TILE, a.ch - R0), tw = min(TILE, a.cw - C0);
  const unsigned char* base = a.frames[n];
  const int flags = a.desc[3 * n + 2];
  // the descriptors are trusted to be in range; clamping keeps a wrong one inside its frame all the same
  const int y0 = min(max(a.desc[3 * n], 0), a.H - a.ch), x0 = min(max(a.desc[3 * n + 1], 0), a.W - a.cw);
  const bool hf = flags & 1, vf = flags & 2, rot = (flags & 4) && a.ch == a.cw;

  // crop rows i0 .. i0 + ni and columns j0 .. j0 + nj show in this tile; they are source rows sy0 .. and columns sx0 .., ascending
  const int i0 = rot ? C0 : R0, ni = rot ? tw : th, j0 = rot ? R0 : C0, nj = rot ? th : tw;
  const int sy0 = y0 + (vf ? a.ch - i0 - ni : i0), sx0 = x0 + (hf ? a.cw - j0 - nj : j0);

  if (a.mode == CB_INTER_DWORDS) {
    // a source row is one run of 3W bytes; byte b of it is channel b % 3 of pixel b / 3.  All rows start 4-byte-congruent.
    const int bs = 3 * sx0, be = 3 * (sx0 + nj);
    const int b0 = bs - (int)(((uintptr_t)base + (uintptr_t)((long long)sy0 * a.sr) + (uintptr_t)bs) & 3);
    const int ndw = (be - b0 + 3) >> 2;
    for (int i = tid; i < ni * IDW; i += 256) {
      const int r = i / IDW, d = i - r * IDW;
      if (d >= ndw) continue;
      const unsigned char* row = base + (long long)(sy0 + r) * a.sr;
      const int b = b0 + 4 * d;
      unsigned int word = 0;
      if (b >= 0 && b + 4 <= 3 * a.W) {
        word = *reinterpret_cast<const unsigned int*>(row + b);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (b + q >= bs && b + q < be) word |= (unsigned int)row[b + q] << (8 * q);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rel = b + q - bs;
        if (rel >= 0 && b + q < be) {
          const int px = (int)((unsigned int)rel / 3u);
          tile[(rel - 3 * px) * PLANE + r * PITCH + px] = (unsigned char)(word >> (8 * q));
        }
      }
    }
  } else if (a.mode == CB_PLANAR_DWORDS) {
    // three runs of pixels per source row; the rows of one channel start 4-byte-congruent
    for (int i = tid; i < ni * 3 * PDW; i += 256) {
      const int d = i % PDW, c = (i / PDW) % 3, r = i / (3 * PDW);
      const unsigned char* row = base + c * a.sc + (long long)(sy0 + r) * a.sr;
      const int x = sx0 - (int)(((uintptr_t)row + (uintptr_t)sx0) & 3) + 4 * d;
      if (x >= sx0 + nj) continue;
      unsigned int word = 0;
      if (x >= 0 && x + 4 <= a.W) {
        word = *reinterpret_cast<const unsigned int*>(row + x);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (x + q >= sx0 && x + q < sx0 + nj) word |= (unsigned int)row[x + q] << (8 * q);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rel = x + q - sx0;
        if (rel >= 0 && rel < nj) tile[c * PLANE + r * PITCH + rel] = (unsigned char)(word >> (8 * q));
      }
    }
  } else {
    // any strides, byte by byte; consecutive lanes follow the store's fastest axis
    const bool ch_fast = a.sc < a.sp;
    for (int i = tid; i < ni * nj * 3; i += 256) {
      const int r = i / (3 * nj), k = i - r * 3 * nj;
      const int c = ch_fast ? k % 3 : k / nj, x = ch_fast ? k / 3 : k % nj;
      tile[c * PLANE + r * PITCH + x] = base[c * a.sc + (long long)(sy0 + r) * a.sr + (long long)(sx0 + x) * a.sp];
    }
  }
  __syncthreads();

  // output (r, c) of the tile shows plane byte (row, column) = (ii or ni-1-ii, jj or nj-1-jj) with (ii, jj) = rot ? (c, r) : (r, c)
  const int dy = vf ? -PITCH : PITCH, dx = hf ? -1 : 1;
  const int origin = (vf ? (ni - 1) * PITCH : 0) + (hf ? nj - 1 : 0);
  const int dr = rot ? dx : dy, dc = rot ? dy : dx;

  const int r = tid >> 3, c = (tid & 7) * 4;
  if (r >= th || c >= tw) return;
  const int esize = a.out_type == VMG_CROP_U8 ? 1 : a.out_type == VMG_CROP_BF16 ? 2 : 4;
  const int at = origin + r * dr + c * dc;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const unsigned char* p = tile + (a.crev ? 2 - k : k) * PLANE + at;
    const long long idx = (((long long)n * 3 + k) * a.ch + R0 + r) * a.cw + C0 + c;
    const uintptr_t addr = (uintptr_t)a.out + (uintptr_t)idx * esize;
    if (c + 4 <= tw && (addr & (uintptr_t)(4 * esize - 1)) == 0) {
      const unsigned int b0 = p[0], b1 = p[dc], b2 = p[2 * dc], b3 = p[3 * dc];
      if (a.out_type == VMG_CROP_U8) {
        *reinterpret_cast<unsigned int*>(addr) = b0 | b1 << 8 | b2 << 16 | b3 << 24;
      } else {
        const float v[4] = {__fdiv_rn((float)b0, 255.0f), __fdiv_rn((float)b1, 255.0f), __fdiv_rn((float)b2, 255.0f), __fdiv_rn((float)b3, 255.0f)};
        if (a.out_type == VMG_CROP_F32)
          store4(reinterpret_cast<float*>(addr), v);
        else
          store4(reinterpret_cast<bf16*>(addr), v);
      }
    } else {
      for (int q = 0; q < 4 && c + q < tw; ++q) store1(a.out, a.out_type, idx + q, p[q * dc]);
    }
  }
}

}  // namespace

extern "C" int vmg_crop_batch(const void* const* frames, const int64_t* strides, const int* desc, int N, int H, int W, int ch, int cw,
                              int channel_reverse, int out_type, void* out, void* stream) {
  VMG_CHECK(frames && strides && desc && out, "crop_batch: null argument");
  VMG_CHECK(N > 0, "crop_batch: at least one crop expected, got %d", N);
  VMG_CHECK(H > 0 && W > 0 && H <= (1 << 16) && W <= (1 << 16), "crop_batch: frame size %d x %d out of range", H, W);
  VMG_CHECK(ch > 0 && cw > 0, "crop_batch: empty crop %d x %d", ch, cw);
  VMG_CHECK(ch <= H && cw <= W, "crop_batch: a %d x %d crop is larger than the %d x %d frame", ch, cw, H, W);
  VMG_CHECK(out_type >= VMG_CROP_U8 && out_type <= VMG_CROP_BF16, "crop_batch: unknown output type %d", out_type);
  const int esize = out_type == VMG_CROP_U8 ? 1 : out_type == VMG_CROP_BF16 ? 2 : 4;
  VMG_CHECK(((uintptr_t)out & (esize - 1)) == 0, "crop_batch: misaligned output");
  for (int i = 0; i < 3; ++i) VMG_CHECK(strides[i] >= 0, "crop_batch: negative stride");
  const int tx = cdiv(cw, TILE), ty = cdiv(ch, TILE);
  const int64_t tiles = (int64_t)N * tx * ty;
  VMG_CHECK(tiles < (1 << 24), "crop_batch: %lld tiles in one call, at most %d", (long long)tiles, (1 << 24) - 1);

  CropArgs a;
  a.frames = reinterpret_cast<const unsigned char* const*>(frames);
  a.desc = desc;
  a.sr = strides[0], a.sp = strides[1], a.sc = strides[2];
  a.H = H, a.W = W, a.ch = ch, a.cw = cw, a.tx = tx, a.ty = ty;
  a.crev = channel_reverse != 0;
  a.out_type = out_type;
  a.out = out;
  // rows that start multiples of 4 bytes apart are fetched as dwords, wherever the frames themselves start
  a.mode = CB_BYTES;
  if (a.sr % 4 == 0 && a.sp == 1) a.mode = CB_PLANAR_DWORDS;
  if (a.sr % 4 == 0 && a.sp == 3 && a.sc == 1) a.mode = CB_INTER_DWORDS;

  hipLaunchKernelGGL(crop_batch_kernel, dim3((unsigned int)tiles), dim3(256), 0, (hipStream_t)stream, a);
  VMG_LAUNCH_CHECK();
  return 0;
}
