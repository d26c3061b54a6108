// Optimizer-side HBM-streaming kernels (gfx950): Adam + EMA in one pass, the reference-exact
// multi-tensor EMA, and the bf16 weight images the GEMMs read.
//
//  es_adam_ema_step    torch.optim.Adam(betas=(0.9,0.999), eps=1e-8, weight_decay=0)
//                      (code/optimizer.py:50-51, single-tensor update order) fused with the EMA
//                      e <- d*e + (1-d)*theta (code/ema.py:51-59) over the flat parameter buffer:
//                      one read of (p, g, m, v, e), one write of (p, m, v, e) per parameter.
//  es_adamw_ema_step   torch.optim.AdamW (code/optimizer.py:47-49) and
//  es_sgd_ema_step     torch.optim.SGD(momentum, nesterov) (code/optimizer.py:43-46), each fused with the same
//                      EMA blend, with per-param-group lr / weight decay from a class map (one byte per
//                      64 floats); frozen parameters and padding are skipped.
//  es_ema_update_multi ModelEMA.update over an arbitrary list of state_dict tensors, fp32 and
//                      int64 (BatchNorm num_batches_tracked: blended in fp32, truncated on copy_).
//  es_pack_weights     fp32 master [N,K] -> bf16 [N,K] (forward operand) and bf16 [K,N] (dgrad
//                      operand, so dgrad is also an NT GEMM), one launch for every matrix.
// The reference evaluates `d*e + (1-d)*m` as three separately rounded fp32 ops (no FMA);
// `#pragma clang fp contract(off)` keeps that order bit-for-bit here.
#include "common.h"

namespace {

__global__ void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                float* __restrict__ v, float* __restrict__ e, long n, float one_minus_b1, float b2,
                                float one_minus_b2, float neg_step, float bc2_sqrt, float eps, float decay,
                                float one_minus_decay, float grad_scale) {
#pragma clang fp contract(off)
  const long n4 = n >> 2;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f32x4 pv = ((f32x4*)p)[i], gv = ((const f32x4*)g)[i], mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
    if (grad_scale != 1.0f) gv *= grad_scale;  // data-parallel mean of summed grads
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // exp_avg.lerp_(grad, 1-beta1)  (weight < 0.5 branch: self + w*(end-self))
      mv[k] = mv[k] + one_minus_b1 * (gv[k] - mv[k]);
      // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2)
      vv[k] = vv[k] * b2 + one_minus_b2 * gv[k] * gv[k];
      // denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps); p.addcdiv_(m, denom, -step)
      const float denom = sqrtf(vv[k]) / bc2_sqrt + eps;
      pv[k] = pv[k] + neg_step * (mv[k] / denom);
    }
    ((f32x4*)p)[i] = pv;
    ((f32x4*)m)[i] = mv;
    ((f32x4*)v)[i] = vv;
    if (e) {
      f32x4 ev = ((f32x4*)e)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) ev[k] = decay * ev[k] + one_minus_decay * pv[k];
      ((f32x4*)e)[i] = ev;
    }
  }
}

// The two weight-decaying rules below take a class map: one byte per 64-float granule of the flat buffer
// (every parameter starts at a multiple of 64 floats), 0 = not trained (frozen parameter or alignment
// padding), 1 = param group 0, 2 = param group 1.  A granule is 16 lanes x one float4, so a vector never
// straddles a class boundary.  Class-0 granules load no gradient or moment and store nothing but the EMA:
// a frozen parameter keeps its bits under weight decay.  The EMA blend runs for every element (ModelEMA.update
// blends frozen parameters too), reading p alone where the class is 0.

// The classes of the four granules a wave's 64 float4 cover (float4 index i, wave-uniform i >> 6), one per byte,
// as one scalar load: the map costs the vector memory path nothing.  Granules past the map's end read as 0.
__device__ __forceinline__ unsigned class_word(const uint8_t* __restrict__ cls, long i, long ng) {
  const long w = __builtin_amdgcn_readfirstlane((int)(i >> 6));
  if (4 * w + 4 <= ng) return ((const unsigned*)cls)[w];
  unsigned r = 0;
  for (int k = 0; k < 4; ++k)
    if (4 * w + k < ng) r |= (unsigned)cls[4 * w + k] << (8 * k);
  return r;
}

__device__ __forceinline__ f32x4 ema_blend(f32x4 ev, f32x4 pv, float decay, float one_minus_decay) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 4; ++k) ev[k] = decay * ev[k] + one_minus_decay * pv[k];
  return ev;
}

// torch.optim.AdamW, single-tensor order: p *= 1 - lr*wd, then adam_ema_kernel's arithmetic.
__global__ void adamw_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                 float* __restrict__ v, float* __restrict__ e, const uint8_t* __restrict__ cls,
                                 long n, float one_minus_b1, float b2, float one_minus_b2, float neg_step0,
                                 float neg_step1, float decay_mul0, float decay_mul1, float bc2_sqrt, float eps,
                                 float decay, float one_minus_decay, float grad_scale) {
#pragma clang fp contract(off)
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const long ng = n >> 6;
  const int lane_shift = (threadIdx.x & 0x30) >> 1;  // this lane's granule of the wave's four, in bits
  unsigned word = class_word(cls, i, ng);
  for (; i < n4; i += stride) {
    const int c = (word >> lane_shift) & 0xff;
    const bool trained = c == 1 || c == 2;
    const bool first = c == 1;
    // the next round's classes are fetched beside this round's vectors (index clamped: the lanes that go on
    // are the wave's first ones, whose next index is in range)
    word = class_word(cls, min(i + stride, n4 - 1), ng);
    if (trained) {
      f32x4 pv = ((f32x4*)p)[i];
      f32x4 ev = e ? ((f32x4*)e)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 gv = ((const f32x4*)g)[i], mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
      const float neg_step = first ? neg_step0 : neg_step1;
      const float decay_mul = first ? decay_mul0 : decay_mul1;
      if (grad_scale != 1.0f) gv *= grad_scale;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        pv[k] = pv[k] * decay_mul;  // param.mul_(1 - lr * weight_decay)
        mv[k] = mv[k] + one_minus_b1 * (gv[k] - mv[k]);
        vv[k] = vv[k] * b2 + one_minus_b2 * gv[k] * gv[k];
        const float denom = sqrtf(vv[k]) / bc2_sqrt + eps;
        pv[k] = pv[k] + neg_step * (mv[k] / denom);
      }
      ((f32x4*)p)[i] = pv;
      ((f32x4*)m)[i] = mv;
      ((f32x4*)v)[i] = vv;
      if (e) ((f32x4*)e)[i] = ema_blend(ev, pv, decay, one_minus_decay);
    } else if (e) {  // frozen or padding: the EMA alone
      const f32x4 pv = ((const f32x4*)p)[i], ev = ((f32x4*)e)[i];
      ((f32x4*)e)[i] = ema_blend(ev, pv, decay, one_minus_decay);
    }
  }
}

// torch.optim.SGD (dampening 0), single-tensor order: d = g + wd*p; buf = buf*momentum + d;
// u = nesterov ? d + momentum*buf : buf; p += -lr*u.  A zero buf makes the first step's buf = d, as torch's clone.
__global__ void sgd_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                               float* __restrict__ e, const uint8_t* __restrict__ cls, long n, float momentum,
                               float neg_lr0, float neg_lr1, float wd0, float wd1, int nesterov, float decay,
                               float one_minus_decay, float grad_scale) {
#pragma clang fp contract(off)
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const long ng = n >> 6;
  const int lane_shift = (threadIdx.x & 0x30) >> 1;  // this lane's granule of the wave's four, in bits
  unsigned word = class_word(cls, i, ng);
  for (; i < n4; i += stride) {
    const int c = (word >> lane_shift) & 0xff;
    const bool trained = c == 1 || c == 2;
    const bool first = c == 1;
    // the next round's classes are fetched beside this round's vectors (index clamped: the lanes that go on
    // are the wave's first ones, whose next index is in range)
    word = class_word(cls, min(i + stride, n4 - 1), ng);
    if (trained) {
      f32x4 pv = ((f32x4*)p)[i];
      f32x4 ev = e ? ((f32x4*)e)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
      const f32x4 gv = ((const f32x4*)g)[i];
      f32x4 bv = ((f32x4*)buf)[i];
      const float neg_lr = first ? neg_lr0 : neg_lr1;
      const float wd = first ? wd0 : wd1;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float d = gv[k] * grad_scale;
        if (wd != 0.0f) d = d + wd * pv[k];  // torch adds nothing at weight_decay 0
        bv[k] = bv[k] * momentum + d;
        const float u = nesterov ? d + momentum * bv[k] : bv[k];
        pv[k] = pv[k] + neg_lr * u;
      }
      ((f32x4*)p)[i] = pv;
      ((f32x4*)buf)[i] = bv;
      if (e) ((f32x4*)e)[i] = ema_blend(ev, pv, decay, one_minus_decay);
    } else if (e) {  // frozen or padding: the EMA alone
      const f32x4 pv = ((const f32x4*)p)[i], ev = ((f32x4*)e)[i];
      ((f32x4*)e)[i] = ema_blend(ev, pv, decay, one_minus_decay);
    }
  }
}

struct EmaEntry {
  void* e; const void* m; long n; int dtype; int pad;  // dtype 0 = fp32, 1 = int64
};

// chunk table: (entry, start) pairs, one block per chunk of up to 4096 elements
__global__ void ema_multi_kernel(const EmaEntry* __restrict__ tab, const int2* __restrict__ chunks, float decay,
                                 float one_minus_decay) {
#pragma clang fp contract(off)
  const int2 ch = chunks[blockIdx.x];
  const EmaEntry en = tab[ch.x];
  const long s = (long)ch.y * 4096;
  const long end = min(s + 4096, en.n);
  for (long i = s + threadIdx.x; i < end; i += blockDim.x) {
    if (en.dtype == 0) {
      float* e = (float*)en.e;
      const float mv = ((const float*)en.m)[i];
      e[i] = decay * e[i] + one_minus_decay * mv;
    } else {
      int64_t* e = (int64_t*)en.e;
      const float r = decay * (float)e[i] + one_minus_decay * (float)((const int64_t*)en.m)[i];
      e[i] = (int64_t)r;  // copy_ into an integer tensor truncates toward zero
    }
  }
}

struct PackEntry {
  long src;     // float offset into the flat parameter buffer
  bf16* dst;    // [N][K] or null
  bf16* dstT;   // [K][N] or null
  int N, K;
};

// grid.y = matrix, grid.x strides over 64x64 tiles of that matrix.  N, K multiples of 4 (every ViT / Conformer
// Linear): 16-B loads of the fp32 master rows, 8-B bf16 stores of W rows and, through the LDS tile, of W^T rows;
// otherwise element-wise.
__global__ void pack_kernel(const float* __restrict__ flat, const PackEntry* __restrict__ tab) {
  __shared__ float tile[64][65];
  const PackEntry en = tab[blockIdx.y];
  const int tn = (en.N + 63) / 64, tk = (en.K + 63) / 64;
  const float* src = flat + en.src;
  const bool vec = (en.N % 4 == 0) && (en.K % 4 == 0);
  typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
  for (int t = blockIdx.x; t < tn * tk; t += gridDim.x) {
    const int n0 = (t / tk) * 64, k0 = (t % tk) * 64;
    if (vec) {
      for (int i = threadIdx.x; i < 64 * 16; i += blockDim.x) {
        const int rr = i / 16, c4 = (i % 16) * 4;
        const int n = n0 + rr, k = k0 + c4;
        const bool ok = n < en.N && k < en.K;
        const f32x4 x = ok ? *(const f32x4*)(src + (size_t)n * en.K + k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) tile[rr][c4 + j] = x[j];
        if (en.dst && ok)
          *(bf16x4_t*)(en.dst + (size_t)n * en.K + k) = bf16x4_t{(bf16)x[0], (bf16)x[1], (bf16)x[2], (bf16)x[3]};
      }
      __syncthreads();
      if (en.dstT) {
        for (int i = threadIdx.x; i < 64 * 16; i += blockDim.x) {
          const int kk = i / 16, n4 = (i % 16) * 4;
          const int n = n0 + n4, k = k0 + kk;
          if (n < en.N && k < en.K)
            *(bf16x4_t*)(en.dstT + (size_t)k * en.N + n) =
                bf16x4_t{(bf16)tile[n4][kk], (bf16)tile[n4 + 1][kk], (bf16)tile[n4 + 2][kk], (bf16)tile[n4 + 3][kk]};
        }
      }
    } else {
      for (int i = threadIdx.x; i < 64 * 64; i += blockDim.x) {
        const int rr = i / 64, cc = i % 64;
        const int n = n0 + rr, k = k0 + cc;
        const float x = (n < en.N && k < en.K) ? src[(size_t)n * en.K + k] : 0.f;
        tile[rr][cc] = x;
        if (en.dst && n < en.N && k < en.K) en.dst[(size_t)n * en.K + k] = (bf16)x;
      }
      __syncthreads();
      if (en.dstT) {
        for (int i = threadIdx.x; i < 64 * 64; i += blockDim.x) {
          const int kk = i / 64, nn = i % 64;
          const int n = n0 + nn, k = k0 + kk;
          if (n < en.N && k < en.K) en.dstT[(size_t)k * en.N + n] = (bf16)tile[nn][kk];
        }
      }
    }
    __syncthreads();
  }
}

__global__ void cast_kernel(const float* __restrict__ x, bf16* __restrict__ y, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    y[i] = (bf16)x[i];
}

// y += x over n floats (n % 4 == 0, 16-byte aligned): the two-lane backward's second flat gradient
__global__ void add_f32_kernel(float* __restrict__ y, const float* __restrict__ x, long n4) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f32x4 a = ((const f32x4*)y)[i];
    a += ((const f32x4*)x)[i];
    ((f32x4*)y)[i] = a;
  }
}

}  // namespace

extern "C" {

int es_add_f32(float* y, const float* x, long n, hipStream_t stream) {
  if (n <= 0 || n % 4) return ES_BAD_SHAPE;
  if (!y || !x || ((uintptr_t)y & 15) || ((uintptr_t)x & 15)) return ES_BAD_ARG;
  long grid = (n / 4 + 255) / 256;
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(add_f32_kernel, (int)grid, 256, 0, stream, y, x, n / 4);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

int es_cast_f32_bf16(const float* x, void* y, long n, hipStream_t stream) {
  if (n <= 0) return ES_BAD_SHAPE;
  long grid = (n + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(cast_kernel, (int)grid, 256, 0, stream, x, (bf16*)y, n);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// n % 4 == 0 and 16-byte aligned buffers.  neg_step = -lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t)
// (host computes them in double exactly as torch.optim.Adam does).  ema may be null.
int es_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, long n, float beta1, float beta2,
                     float eps, float neg_step, float bc2_sqrt, float decay, float one_minus_decay,
                     float grad_scale, hipStream_t stream) {
  if (n <= 0 || n % 4) return ES_BAD_SHAPE;
  if (!p || !g || !m || !v) return ES_BAD_ARG;
  long grid = (n / 4 + 255) / 256;
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(adam_ema_kernel, (int)grid, 256, 0, stream, p, g, m, v, ema, n, 1.0f - beta1, beta2,
                     1.0f - beta2, neg_step, bc2_sqrt, eps, decay, one_minus_decay, grad_scale);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

static bool misaligned16(const void* a) { return ((uintptr_t)a & 15) != 0; }

// n % 64 == 0, 16-byte aligned float buffers, cls: n / 64 bytes, 4-byte aligned (0 untrained, 1 group 0, 2 group 1).
// neg_step{0,1} = -lr_c / (1 - beta1^t), decay_mul{0,1} = (float)(1 - lr_c * wd_c), both computed in double by
// the host as torch.optim.AdamW does.  So are one_minus_beta{1,2} = (float)(1 - beta), the weights torch hands
// its lerp_ / addcmul_: 1.0f - 0.999f in fp32 is 1.3e-5 (relative) off (float)0.001, and exp_avg_sq with it.
// A complement that does not belong to its beta is refused.  ema may be null.
int es_adamw_ema_step(float* p, const float* g, float* m, float* v, float* ema, const uint8_t* cls, long n,
                      float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps,
                      float bc2_sqrt, float neg_step0, float neg_step1, float decay_mul0, float decay_mul1,
                      float decay, float one_minus_decay, float grad_scale, hipStream_t stream) {
  if (n <= 0 || n % 64 || n >= (1L << 38)) return ES_BAD_SHAPE;
  if (!p || !g || !m || !v || !cls) return ES_BAD_ARG;
  if ((uintptr_t)cls & 3) return ES_BAD_ARG;  // read as 32-bit words, four granules each
  if (misaligned16(p) || misaligned16(g) || misaligned16(m) || misaligned16(v) || misaligned16(ema))
    return ES_BAD_ARG;
  if (!(fabsf(1.0f - beta1 - one_minus_beta1) <= 1e-6f) || !(fabsf(1.0f - beta2 - one_minus_beta2) <= 1e-6f))
    return ES_BAD_ARG;
  long grid = (n / 4 + 255) / 256;
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(adamw_ema_kernel, (int)grid, 256, 0, stream, p, g, m, v, ema, cls, n, one_minus_beta1, beta2,
                     one_minus_beta2, neg_step0, neg_step1, decay_mul0, decay_mul1, bc2_sqrt, eps, decay,
                     one_minus_decay, grad_scale);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// The same contract; buf is the momentum buffer (zeros before the first step), neg_lr{0,1} = -lr_c.
int es_sgd_ema_step(float* p, const float* g, float* buf, float* ema, const uint8_t* cls, long n, float momentum,
                    float neg_lr0, float neg_lr1, float wd0, float wd1, int nesterov, float decay,
                    float one_minus_decay, float grad_scale, hipStream_t stream) {
  if (n <= 0 || n % 64 || n >= (1L << 38)) return ES_BAD_SHAPE;
  if (!p || !g || !buf || !cls) return ES_BAD_ARG;
  if ((uintptr_t)cls & 3) return ES_BAD_ARG;  // read as 32-bit words, four granules each
  if (misaligned16(p) || misaligned16(g) || misaligned16(buf) || misaligned16(ema)) return ES_BAD_ARG;
  long grid = (n / 4 + 255) / 256;
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(sgd_ema_kernel, (int)grid, 256, 0, stream, p, g, buf, ema, cls, n, momentum, neg_lr0, neg_lr1,
                     wd0, wd1, nesterov, decay, one_minus_decay, grad_scale);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// entries: device array of {e, m, n, dtype}; chunks: device array of int2 {entry, chunk_index}
int es_ema_update_multi(const void* entries, const void* chunks, int nchunks, float decay, float one_minus_decay,
                        hipStream_t stream) {
  if (nchunks <= 0) return ES_BAD_SHAPE;
  if (!entries || !chunks) return ES_BAD_ARG;
  hipLaunchKernelGGL(ema_multi_kernel, nchunks, 256, 0, stream, (const EmaEntry*)entries, (const int2*)chunks,
                     decay, one_minus_decay);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

int es_ema_entry_size(void) { return (int)sizeof(EmaEntry); }
int es_pack_entry_size(void) { return (int)sizeof(PackEntry); }

int es_pack_weights(const float* flat, const void* entries, int nmat, hipStream_t stream) {
  if (nmat <= 0) return ES_BAD_SHAPE;
  if (!flat || !entries) return ES_BAD_ARG;
  dim3 grid(128, nmat);
  hipLaunchKernelGGL(pack_kernel, grid, 256, 0, stream, flat, (const PackEntry*)entries);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

}  // extern "C"
