// Fused FixMatch loss kernels: forward value AND d(loss)/d(logits) in one launch (gfx950).
//
//  es_fm_consistency_fwd_bwd  code/loss.py:126-164 (consistency_loss, name='ce', hard labels):
//      p = softmax(detach(l_w)); (max_p, idx) = max(p, -1)   [first index on ties]
//      mask = (max_p >= tau)                                 [inclusive]
//      loss = mean_i( CE(l_s[i], idx[i]) * mask[i] ),  mask_mean = mean(mask)   (T unused)
//      d loss / d l_s[i][c] = mask[i] * (softmax(l_s[i])_c - [c == idx[i]]) * grad_scale
//  es_poly_ce_fwd_bwd         code/loss.py:103-114,308-364 (PolyLoss, softmax=True, epsilon=2):
//      loss = mean_i( w[y_i] * CE_i + eps * (1 - p_i[y_i]) )   (plain mean, not weight-normalised)
//      d/d l[i][c] = grad_scale * (w[y_i] + eps * p_i[y_i]) * (p_i[c] - [c == y_i])
//  es_triplet_fwd_bwd         code/loss.py:170-190 (TripletLoss, alpha = 0.7) on z = [anchors; positives; negatives]
//  es_softmax_predict         code/supervised.py:258-266 (inference: argmax, max probability, thresholded label)
// The logits are tiny ([448,23] / [64,23]); one workgroup handles all rows, staging each row's
// logits in registers, and emits int32 pseudo-labels, the uint8 mask, per-row losses and the two
// means -- no host sync and no intermediate tensors.
#include "common.h"

namespace {

constexpr int MAXC = 64;

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = warp_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float s = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
  return s;
}

__global__ __launch_bounds__(256) void fm_consistency_kernel(const float* __restrict__ lw, int ldw,
                                                             const float* __restrict__ ls, int lds_, int n, int C,
                                                             float tau, float grad_scale, int* __restrict__ pl,
                                                             uint8_t* __restrict__ mask_out,
                                                             float* __restrict__ row_loss, float* __restrict__ dls,
                                                             int lddls, float* __restrict__ out) {
  __shared__ float red[16];
  float sum_loss = 0.f, sum_mask = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    // pseudo-label from the weak view (logits re-read from L1 instead of a private array)
    const float* wr = lw + (size_t)i * ldw;
    const float* sr = ls + (size_t)i * lds_;
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, wr[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += __expf(wr[c] - mx);
    const float inv = 1.0f / se;
    float pmax = -1.f;
    int idx = 0;
    for (int c = 0; c < C; ++c) {
      const float p = __expf(wr[c] - mx) * inv;
      if (p > pmax) {
        pmax = p;
        idx = c;
      }
    }
    const float m = pmax >= tau ? 1.f : 0.f;
    // CE of the strong view against idx
    float mxs = -INFINITY;
    for (int c = 0; c < C; ++c) mxs = fmaxf(mxs, sr[c]);
    float ses = 0.f;
    for (int c = 0; c < C; ++c) ses += __expf(sr[c] - mxs);
    const float lse = mxs + __logf(ses);
    const float ce = lse - sr[idx];
    const float rl = ce * m;
    const float invs = 1.0f / ses;
    for (int c = 0; c < C; ++c) {
      const float p = __expf(sr[c] - mxs) * invs;
      dls[(size_t)i * lddls + c] = m * (p - (c == idx ? 1.f : 0.f)) * grad_scale;
    }
    if (pl) pl[i] = idx;
    if (mask_out) mask_out[i] = (uint8_t)m;
    if (row_loss) row_loss[i] = rl;
    sum_loss += rl;
    sum_mask += m;
  }
  sum_loss = block_sum(sum_loss, red);
  sum_mask = block_sum(sum_mask, red);
  if (threadIdx.x == 0) {
    out[0] = sum_loss / (float)n;
    out[1] = sum_mask / (float)n;
  }
}

__global__ __launch_bounds__(256) void poly_ce_kernel(const float* __restrict__ l, int ldl,
                                                      const int64_t* __restrict__ y, const float* __restrict__ w,
                                                      int n, int C, float eps, float grad_scale,
                                                      float* __restrict__ dl, int lddl, float* __restrict__ out) {
  __shared__ float red[16];
  float sum = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float* lr = l + (size_t)i * ldl;
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, lr[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += __expf(lr[c] - mx);
    const float lse = mx + __logf(se);
    const int yi = (int)y[i];
    if ((unsigned)yi >= (unsigned)C) {  // invalid target: NaN loss, no gradient, no out-of-range read
      sum += __int_as_float(0x7fc00000);
      for (int c = 0; c < C; ++c) dl[(size_t)i * lddl + c] = 0.f;
      continue;
    }
    const float wy = w ? w[yi] : 1.f;
    const float py = __expf(lr[yi] - lse);
    sum += wy * (lse - lr[yi]) + eps * (1.f - py);
    const float coef = grad_scale * (wy + eps * py);
    for (int c = 0; c < C; ++c) {
      const float p = __expf(lr[c] - lse);
      dl[(size_t)i * lddl + c] = coef * (p - (c == yi ? 1.f : 0.f));
    }
  }
  sum = block_sum(sum, red);
  if (threadIdx.x == 0) out[0] = sum / (float)n;
}

// F.cross_entropy(logits, y, weight=w, reduction='mean') = sum_i w[y_i] l_i / sum_i w[y_i]
// (code/loss.py:118, the SemiFormer heads' loss, code/semiformer.py:125-126); one workgroup.
__global__ __launch_bounds__(256) void ce_weighted_kernel(const float* __restrict__ l, int ldl,
                                                          const int64_t* __restrict__ y, const float* __restrict__ w,
                                                          const float* __restrict__ wsum_global, int n, int C,
                                                          float grad_scale, float* __restrict__ dl, int lddl,
                                                          float* __restrict__ out) {
  __shared__ float red[16];
  float ws = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int yi = (int)y[i];
    ws += (unsigned)yi >= (unsigned)C ? __int_as_float(0x7fc00000) : (w ? w[yi] : 1.f);
  }
  float W = block_sum(ws, red);
  __syncthreads();
  if (wsum_global) W = *wsum_global;  // the whole batch's weight sum over every rank (data-parallel step)
  const float invW = 1.0f / W;
  float sum = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float* lr = l + (size_t)i * ldl;
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, lr[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += __expf(lr[c] - mx);
    const float lse = mx + __logf(se);
    const int yi = (int)y[i];
    if ((unsigned)yi >= (unsigned)C) {  // invalid target: NaN loss (via the weight sum), no gradient
      for (int c = 0; c < C; ++c) dl[(size_t)i * lddl + c] = 0.f;
      continue;
    }
    const float wy = w ? w[yi] : 1.f;
    sum += wy * (lse - lr[yi]);
    const float coef = grad_scale * wy * invW;
    for (int c = 0; c < C; ++c) {
      const float p = __expf(lr[c] - lse);
      dl[(size_t)i * lddl + c] = coef * (p - (c == yi ? 1.f : 0.f));
    }
  }
  sum = block_sum(sum, red);
  if (threadIdx.x == 0) out[0] = sum * invW;
}

__global__ __launch_bounds__(256) void ce_weight_sum_kernel(const int64_t* __restrict__ y, const float* __restrict__ w,
                                                            int n, int C, float* __restrict__ out) {
  __shared__ float red[16];
  float ws = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int yi = (int)y[i];
    ws += (unsigned)yi >= (unsigned)C ? __int_as_float(0x7fc00000) : (w ? w[yi] : 1.f);
  }
  ws = block_sum(ws, red);
  if (threadIdx.x == 0) out[0] = ws;
}

// TripletLoss (code/loss.py:170-190) on the L2-normalised embeddings, value and gradient; one workgroup,
// one wave per triplet (wave w takes triplets w, w + nw, ...).  Lanes stride the L columns twice: the
// squared distances, then -- the rows still in L1 -- the three gradient rows.  The four means are summed per
// wave in triplet order and across waves in wave order: no atomics, the same bits on every launch.
constexpr int TRIPLET_THREADS = 1024;

__global__ __launch_bounds__(TRIPLET_THREADS) void triplet_kernel(const float* __restrict__ z, int ldz, int bs, int L,
                                                                  float alpha, float grad_scale,
                                                                  float* __restrict__ dz, int lddz,
                                                                  float* __restrict__ out) {
  __shared__ float red[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  float s_h = 0.f, s_p = 0.f, s_n = 0.f, s_act = 0.f;  // wave-uniform
  for (int i = w; i < bs; i += nw) {
    const float* za = z + (size_t)i * ldz;
    const float* zp = z + (size_t)(bs + i) * ldz;
    const float* zn = z + (size_t)(2 * bs + i) * ldz;
    float sp = 0.f, sn = 0.f;
    for (int k = lane; k < L; k += 64) {
      const float a = za[k], ep = a - zp[k], en = a - zn[k];
      sp = fmaf(ep, ep, sp);
      sn = fmaf(en, en, sn);
    }
    const float dp = sqrtf(warp_sum(sp)), dn = sqrtf(warp_sum(sn));
    const float h = dp - dn + alpha;
    const bool act = h > 0.f;  // h == 0 is inactive
    s_h += act ? h : 0.f;
    s_p += dp;
    s_n += dn;
    s_act += act ? 1.f : 0.f;
    // unit directions scaled by grad_scale; 0 at zero distance (torch.norm's backward) and for h <= 0
    const float cp = act && dp > 0.f ? grad_scale / dp : 0.f;
    const float cn = act && dn > 0.f ? grad_scale / dn : 0.f;
    float* ga = dz + (size_t)i * lddz;
    float* gp = dz + (size_t)(bs + i) * lddz;
    float* gn = dz + (size_t)(2 * bs + i) * lddz;
    for (int k = lane; k < L; k += 64) {
      const float a = za[k], up = (a - zp[k]) * cp, un = (a - zn[k]) * cn;
      ga[k] = up - un;
      gp[k] = -up;
      gn[k] = un;
    }
  }
  const float inv = 1.0f / (float)bs;
  s_h = block_sum(lane == 0 ? s_h : 0.f, red);
  s_p = block_sum(lane == 0 ? s_p : 0.f, red);
  s_n = block_sum(lane == 0 ? s_n : 0.f, red);
  s_act = block_sum(lane == 0 ? s_act : 0.f, red);
  if (threadIdx.x == 0) {
    out[0] = s_h * inv;
    out[1] = s_p * inv;
    out[2] = s_n * inv;
    out[3] = s_act * inv;
  }
}

// softmax argmax / confidence / thresholded label per row (code/supervised.py:238-268, inference): a thread
// per row, grid-stride over the rows.  conf = 1 / sum_c exp(l_c - max): the max's own probability.
__global__ __launch_bounds__(256) void softmax_predict_kernel(const float* __restrict__ l, int ldl, int n, int C,
                                                              float thres, int* __restrict__ pred,
                                                              float* __restrict__ conf, int* __restrict__ label) {
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float* lr = l + (size_t)i * ldl;
    float mx = lr[0];
    int idx = 0;
    for (int c = 1; c < C; ++c) {
      const float v = lr[c];
      if (v > mx) {  // strict: the first index on ties
        mx = v;
        idx = c;
      }
    }
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += __expf(lr[c] - mx);
    const float p = 1.0f / se;
    if (pred) pred[i] = idx;
    if (conf) conf[i] = p;
    if (label) label[i] = p > thres ? idx : 0;
  }
}

}  // namespace

extern "C" {

// out[0] = weighted-mean CE (weights nullable -> plain mean); dl = grad_scale * d(out[0])/d logits
int es_ce_weighted_fwd_bwd(const float* logits, int ldl, const int64_t* targets, const float* weights, int n, int C,
                           float grad_scale, float* dlogits, int lddl, float* out, hipStream_t stream) {
  if (n <= 0 || C <= 0) return ES_BAD_SHAPE;
  if (!logits || !targets || !dlogits || !out) return ES_BAD_ARG;
  hipLaunchKernelGGL(ce_weighted_kernel, 1, 256, 0, stream, logits, ldl, targets, weights, nullptr, n, C, grad_scale,
                     dlogits, lddl, out);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// out[0] = sum_i w[y_i] (the local weight sum of the weighted mean; weights nullable -> n)
int es_ce_weight_sum(const int64_t* targets, const float* weights, int n, int C, float* out, hipStream_t stream) {
  if (n <= 0 || C <= 0) return ES_BAD_SHAPE;
  if (!targets || !out) return ES_BAD_ARG;
  hipLaunchKernelGGL(ce_weight_sum_kernel, 1, 256, 0, stream, targets, weights, n, C, out);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// The data-parallel form: the rows are this rank's shard, *wsum_global the weight sum over every
// rank's rows (es_ce_weight_sum + a SUM all-reduce), so out[0] = this shard's share of the global
// weighted mean, sum_{i in shard} w l_i / W_global, and dl = grad_scale * d(out[0])/d logits.
int es_ce_weighted_fwd_bwd_global(const float* logits, int ldl, const int64_t* targets, const float* weights,
                                  const float* wsum_global, int n, int C, float grad_scale, float* dlogits, int lddl,
                                  float* out, hipStream_t stream) {
  if (n <= 0 || C <= 0) return ES_BAD_SHAPE;
  if (!logits || !targets || !dlogits || !out || !wsum_global) return ES_BAD_ARG;
  hipLaunchKernelGGL(ce_weighted_kernel, 1, 256, 0, stream, logits, ldl, targets, weights, wsum_global, n, C,
                     grad_scale, dlogits, lddl, out);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// out[0] = loss (mean over n of masked CE), out[1] = mask mean.  dls = d(grad_scale*loss*n)/d l_s
// i.e. pass grad_scale = lambda_u / n for d(lambda_u * loss).  pl / mask_out / row_loss nullable.
int es_fm_consistency_fwd_bwd(const float* logits_w, int ldw, const float* logits_s, int lds, int n, int C,
                              float tau, float grad_scale, int* pseudo_label, uint8_t* mask, float* row_loss,
                              float* dlogits_s, int lddls, float* out, hipStream_t stream) {
  if (n <= 0 || C <= 0 || C > MAXC) return ES_BAD_SHAPE;
  if (!logits_w || !logits_s || !dlogits_s || !out) return ES_BAD_ARG;
  hipLaunchKernelGGL(fm_consistency_kernel, 1, 256, 0, stream, logits_w, ldw, logits_s, lds, n, C, tau, grad_scale,
                     pseudo_label, mask, row_loss, dlogits_s, lddls, out);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// out[0] = poly loss (mean over n); dl = grad_scale * n * d(loss)/d l  (grad_scale = 1/n for d loss)
int es_poly_ce_fwd_bwd(const float* logits, int ldl, const int64_t* targets, const float* weights, int n, int C,
                       float epsilon, float grad_scale, float* dlogits, int lddl, float* out, hipStream_t stream) {
  if (n <= 0 || C <= 0 || C > MAXC) return ES_BAD_SHAPE;
  if (!logits || !targets || !dlogits || !out) return ES_BAD_ARG;
  hipLaunchKernelGGL(poly_ce_kernel, 1, 256, 0, stream, logits, ldl, targets, weights, n, C, epsilon, grad_scale,
                     dlogits, lddl, out);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// z [3 bs, L]: anchors, positives, negatives.  h_i = d_p,i - d_n,i + alpha; out = {mean max(h, 0), mean d_p,
// mean d_n, fraction of h > 0}; dz = grad_scale * d(sum_i max(h_i, 0))/dz, every row written (zeros for h <= 0)
int es_triplet_fwd_bwd(const float* z, int ldz, int bs, int L, float alpha, float grad_scale, float* dz, int lddz,
                       float* out, hipStream_t stream) {
  if (bs < 1 || bs > 0x7fffffff / 3 || L < 1 || L > 2048 || ldz < L || lddz < L) return ES_BAD_SHAPE;
  if (!z || !dz || !out) return ES_BAD_ARG;
  hipLaunchKernelGGL(triplet_kernel, 1, TRIPLET_THREADS, 0, stream, z, ldz, bs, L, alpha, grad_scale, dz, lddz, out);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// pred = argmax (first index on ties), conf = max softmax probability, label = conf > thres ? pred : 0;
// each output nullable, not all three
int es_softmax_predict(const float* logits, int ldl, int n, int C, float thres, int* pred, float* conf, int* label,
                       hipStream_t stream) {
  if (n <= 0 || C <= 0 || C > MAXC || ldl < C) return ES_BAD_SHAPE;
  if (!logits || (!pred && !conf && !label)) return ES_BAD_ARG;
  const int blocks = (n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024;
  hipLaunchKernelGGL(softmax_predict_kernel, blocks, 256, 0, stream, logits, ldl, n, C, thres, pred, conf, label);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

}  // extern "C"
