// MorphFC retention decay (reference: Enhanced_MorphFCs_decay.forward, models/function.py:766-768, 779-781: `weight.mul_(gamma)` at EVERY
// call, eval included): W <- W * Gamma applied `reps` times to a list of fp32 weights, one launch per DECAY_MAX_TENSORS tensors.
//   Every element is loaded once, multiplied by its Gamma element `reps` times in a register -- one rounded fp32 multiply after the other,
//   the bits of `reps` separate in-place multiplies -- and stored once.  No power, no squaring: fl(fl(w*g)*g) is not fl(w * fl(g*g)).
//   This file must stay free of fast-math / re-association / denormal-flushing options (the build has none).
// Bandwidth-trivial: a few MB of weights and Gamma read, the weights written; the launch latency and, for large `reps`, the dependent
// multiply chain (reps multiplies per element) are what it costs.
#include "common.h"

namespace {

constexpr int DECAY_MAX_TENSORS = 32;   // per launch (kernel-argument table); longer lists take several launches
constexpr int DECAY_MAX_BLOCKS = 1024;  // per tensor; a block strides over its tensor beyond that

struct DecayK {
  float* w[DECAY_MAX_TENSORS];
  const float* g[DECAY_MAX_TENSORS];
  long long n[DECAY_MAX_TENSORS];     // elements
  long long head[DECAY_MAX_TENSORS];  // leading scalars in front of the 16-byte aligned body (== n: no vector body)
  int blk0[DECAY_MAX_TENSORS + 1];    // tensor i owns blocks [blk0[i], blk0[i+1])
  int count, reps;
};

__device__ __forceinline__ float decay_mul(float x, float g, int reps) {
  for (int r = 0; r < reps; ++r) x = x * g;
  return x;
}

__global__ __launch_bounds__(256) void decay_weights_kernel(const DecayK k) {
  int i = 0;
  while (i + 1 < k.count && (int)blockIdx.x >= k.blk0[i + 1]) ++i;
  float* w = k.w[i];
  const float* g = k.g[i];
  const long long n = k.n[i];
  const long long head = k.head[i] < n ? k.head[i] : n;
  const long long nvec = (n - head) / 4;
  const long long tail0 = head + 4 * nvec;  // first element behind the vector body
  const long long lane = (long long)((int)blockIdx.x - k.blk0[i]) * 256 + threadIdx.x;
  const long long stride = (long long)(k.blk0[i + 1] - k.blk0[i]) * 256;
  const int reps = k.reps;
  float4* wv = reinterpret_cast<float4*>(w + head);
  const float4* gv = reinterpret_cast<const float4*>(g + head);
  for (long long v = lane; v < nvec; v += stride) {
    float4 x = wv[v];
    const float4 y = gv[v];
    x.x = decay_mul(x.x, y.x, reps);
    x.y = decay_mul(x.y, y.y, reps);
    x.z = decay_mul(x.z, y.z, reps);
    x.w = decay_mul(x.w, y.w, reps);
    wv[v] = x;
  }
  // the scalars in front of and behind the body: elements [0, head) and [tail0, n)
  const long long nscal = head + (n - tail0);
  for (long long s = lane; s < nscal; s += stride) {
    const long long e = s < head ? s : tail0 + (s - head);
    w[e] = decay_mul(w[e], g[e], reps);
  }
}

}  // namespace

extern "C" int vmg_decay_weights(float* const* w, const float* const* gamma, const int64_t* numel, int count, int n, void* stream) {
  VMG_CHECK(w && gamma && numel && count >= 1 && n >= 1, "decay_weights: a list of at least one tensor and n >= 1 expected");
  for (int i = 0; i < count; ++i)
    VMG_CHECK(w[i] && gamma[i] && numel[i] > 0 && ((uintptr_t)w[i] | (uintptr_t)gamma[i]) % 4 == 0, "decay_weights: tensor %d: null, empty or not a float pointer", i);
  for (int i0 = 0; i0 < count; i0 += DECAY_MAX_TENSORS) {
    DecayK k;
    k.count = count - i0 < DECAY_MAX_TENSORS ? count - i0 : DECAY_MAX_TENSORS;
    k.reps = n;
    int blocks = 0;
    for (int j = 0; j < DECAY_MAX_TENSORS; ++j) {
      k.blk0[j] = blocks;
      if (j >= k.count) {
        k.w[j] = nullptr; k.g[j] = nullptr; k.n[j] = 0; k.head[j] = 0;
        continue;
      }
      k.w[j] = w[i0 + j];
      k.g[j] = gamma[i0 + j];
      k.n[j] = numel[i0 + j];
      // 16-byte vectors need W and Gamma to reach a 16-byte boundary at the same element; otherwise the whole tensor goes element by element
      const int hw = (int)((16 - (uintptr_t)k.w[j] % 16) % 16) / 4, hg = (int)((16 - (uintptr_t)k.g[j] % 16) % 16) / 4;
      const bool vec = hw == hg && k.n[j] >= hw + 4;
      k.head[j] = vec ? hw : k.n[j];
      const long long work = vec ? cdiv64((k.n[j] - hw) / 4, 256) : cdiv64(k.n[j], 256);  // (>= 1; the <= 6 border scalars ride on the first lanes)
      blocks += (int)(work > DECAY_MAX_BLOCKS ? DECAY_MAX_BLOCKS : work);
    }
    k.blk0[DECAY_MAX_TENSORS] = blocks;
    hipLaunchKernelGGL(decay_weights_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, k);
    VMG_LAUNCH_CHECK();
  }
  return 0;
}
