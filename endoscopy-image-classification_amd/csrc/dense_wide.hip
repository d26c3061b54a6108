// The dense head layers at ResNet-50's width (D = 2048: fc.0 2048 -> 512, head_emb.0 2048 -> 3L) as tiled fp32 GEMMs
// on the exact f32-input MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, fp32 in and out).  Same semantics as
// es_dense_fwd / es_dense_bwd (comatch.hip), whose kernels stage 16 x K rows in LDS and walk K (or n) serially per
// thread: sized for D = 384.
//
//   forward   Y [n, N]  = act(X W^T + b) (* keep * keep_scale)        rows n,  columns N, reduction K
//   dX [n, K] (+)= dpre W                                             rows n,  columns K, reduction N
//   dW [N, K]  = dpre^T X;  db [N] = column sums of dpre              rows N,  columns K, reduction n
//   dpre = dY * act'(Yact) (* keep * keep_scale): one elementwise pass into the workspace (as es_dense_bwd)
//
// One kernel serves the three products: C[m][c] = sum_r A(m, r) B(r, c) with strided operands.  A workgroup of four
// waves owns one 32 x 32 tile of C; the reduction is staged through LDS in steps of KT = 32 (8.4 KB, whatever K is),
// wave w taking k = 8w .. 8w + 7 of every step (four MFMAs), and the four waves' accumulators are summed through LDS
// in wave order.  The backward also splits the reduction over gridDim.z towards TARGET_WG workgroups (the forward has
// no workspace to split through: at n = 96 it runs 24 - 72 workgroups and does not fill the GPU):
// the splits write partials to the workspace and a second kernel adds them in split order.  No atomics: the same call
// gives the same bits.  Out-of-range rows, columns and reduction indices are loaded as zeros and never stored.
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TM = 32, TN = 32, KT = 32;  // C tile, reduction step
// LDS row stride (floats).  An MFMA operand read takes base + ij in lanes 0..31 and base + LW + ij in lanes 32..63: with
// LW = 33 that is 63 banks and one 2-way conflict (lane 63 on lane 0's bank); a stride of 32 would read conflict-free
// but put the loader's transposed stores (four r per thread, 8 threads a row) 8 ways on one bank.  Not measured
// either way.
constexpr int LW = KT + 1;
constexpr int MAXD = 4096;                // K, N limit
constexpr int MAXROWS = 65535 * TM;       // n limit: the row tiles are gridDim.y
constexpr int TARGET_WG = 512;            // the backward splits its reduction until about this many workgroups run

enum { MODE_FWD = 0, MODE_DX = 1, MODE_DW = 2 };

struct Epi {
  int mode;
  float* out;
  long ldo;
  const float* bias;
  int act;
  float slope;
  const uint8_t* keep;
  float keep_scale;
  int accumulate;
};

// the value of C[m][c] -> its place in the output (forward: bias, activation, keep mask; dX: = or +=; dW: =)
__device__ __forceinline__ void epilogue(const Epi& e, int m, int c, int C, float v) {
  float* o = e.out + (size_t)m * e.ldo + c;
  if (e.mode == MODE_FWD) {
    if (e.bias) v += e.bias[c];
    if (e.act == 1) v = fmaxf(v, 0.f);
    else if (e.act == 2) v = v > 0.f ? v : v * e.slope;
    if (e.keep) v = v * ((float)e.keep[(size_t)m * C + c] * e.keep_scale);
    *o = v;
  } else if (e.mode == MODE_DX && e.accumulate) {
    *o = *o + v;
  } else {
    *o = v;
  }
}

// C [M, C] = A B over r in [0, R): A(m, r) = A[m * sam + r * sar], B(r, c) = B[r * sbr + c * sbc].
// gridDim = (C tiles, M tiles, splits); split z owns r in [z * rchunk, min(R, (z + 1) * rchunk)), rchunk % KT == 0.
// part != nullptr: the tile goes to part[z][M][C] as is; else through the epilogue.
__global__ __launch_bounds__(256) void gemm_f32_kernel(const float* __restrict__ A, long sam, long sar,
                                                       const float* __restrict__ B, long sbr, long sbc, int M, int C,
                                                       int R, int rchunk, float* __restrict__ part, Epi epi) {
  __shared__ float As[KT * LW];      // [r][m]
  __shared__ float Bs[KT * LW];      // [r][c]
  __shared__ float red[4 * TM * TN];  // the four waves' tiles
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int m0 = blockIdx.y * TM, c0 = blockIdx.x * TN;
  const int rbeg = blockIdx.z * rchunk, rend = min(R, rbeg + rchunk);
  // loader: thread t brings four elements of each operand per step, along the operand's contiguous direction
  const bool a_rc = sar == 1;  // A contiguous along r (else along m)
  const bool b_rc = sbr == 1;  // B contiguous along r (else along c)
  const int lo = t >> 3, l4 = (t & 7) * 4;  // (outer index 0..31, first of four contiguous indices)
  float ra[4], rb[4];
  auto load = [&](int r0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int am = a_rc ? lo : l4 + j, ar = a_rc ? l4 + j : lo;
      const int bc = b_rc ? lo : l4 + j, br = b_rc ? l4 + j : lo;
      const bool aok = m0 + am < M && r0 + ar < rend, bok = c0 + bc < C && r0 + br < rend;
      ra[j] = aok ? A[(size_t)(m0 + am) * sam + (size_t)(r0 + ar) * sar] : 0.f;
      rb[j] = bok ? B[(size_t)(r0 + br) * sbr + (size_t)(c0 + bc) * sbc] : 0.f;
    }
  };
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  if (rbeg < rend) load(rbeg);
  for (int r0 = rbeg; r0 < rend; r0 += KT) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int am = a_rc ? lo : l4 + j, ar = a_rc ? l4 + j : lo;
      const int bc = b_rc ? lo : l4 + j, br = b_rc ? l4 + j : lo;
      As[ar * LW + am] = ra[j];
      Bs[br * LW + bc] = rb[j];
    }
    __syncthreads();
    if (r0 + KT < rend) load(r0 + KT);  // the next step's operands in flight behind this step's MFMAs
    // lane l of 32x32x2: A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]
    const int kk = wave * 8 + (lane >> 5), ij = lane & 31;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(kk + 2 * s) * LW + ij], Bs[(kk + 2 * s) * LW + ij], acc, 0, 0, 0);
    __syncthreads();
  }
  // C/D map: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
    red[wave * (TM * TN) + row * TN + (lane & 31)] = acc[i];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = t + 256 * j, row = e >> 5, col = e & 31;
    const int m = m0 + row, c = c0 + col;
    if (m < M && c < C) {
      const float v = ((red[e] + red[TM * TN + e]) + red[2 * TM * TN + e]) + red[3 * TM * TN + e];
      if (part) part[((size_t)blockIdx.z * M + m) * C + c] = v;
      else epilogue(epi, m, c, C, v);
    }
  }
}

// the splits' partials added in split order, then the epilogue
__global__ void split_reduce_kernel(const float* __restrict__ part, int splits, int M, int C, Epi epi) {
  const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x, MC = (size_t)M * C;
  if (id >= MC) return;
  float v = part[id];
  for (int s = 1; s < splits; ++s) v += part[(size_t)s * MC + id];
  epilogue(epi, (int)(id / C), (int)(id % C), C, v);
}

// dpre[i][c] = dY[i][c] * act'(Yact[i][c]) (* keep * scale), the derivative read off the stored output (comatch.hip's
// dense_dpre_kernel: a dropped or non-positive output passes no gradient, LeakyReLU passes slope)
__global__ void dpre_kernel(const float* __restrict__ dY, int lddy, const float* __restrict__ Yact, int ldya, int act,
                            float slope, const uint8_t* __restrict__ keep, float keep_scale,
                            float* __restrict__ dpre, int n, int N) {
  const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (size_t)n * N) return;
  const int i = (int)(id / N), c = (int)(id % N);
  float g = dY[(size_t)i * lddy + c];
  if (keep) g *= (float)keep[id] * keep_scale;
  if (act) {
    const float y = Yact[(size_t)i * ldya + c];
    if (!(y > 0.f)) g = act == 1 ? 0.f : g * slope;
  }
  dpre[id] = g;
}

// db[c] = sum_i dpre[i][c]: 64 columns per workgroup, four row groups (rows g, g + 4, ...) added in group order
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ dpre, float* __restrict__ db, int n,
                                                     int N) {
  __shared__ float part[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
  float s = 0.f;
  if (c < N)
    for (int i = g; i < n; i += 4) s += dpre[(size_t)i * N + c];
  part[g][threadIdx.x & 63] = s;
  __syncthreads();
  if (g == 0 && c < N) db[c] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
}

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// splits of a reduction of length R for an [M, C] product: enough for about TARGET_WG workgroups, each a whole number
// of KT steps; -> (splits, rchunk)
inline void split_rule(int M, int C, int R, int* splits, int* rchunk) {
  const long tiles = (long)cdiv(M, TM) * cdiv(C, TN);
  const int steps = cdiv(R, KT);
  int s = (int)std::min<long>(steps, std::max<long>(1, (TARGET_WG + tiles - 1) / tiles));
  const int per = cdiv(steps, s);
  *rchunk = per * KT;
  *splits = cdiv(steps, per);
}

inline size_t partial_floats(int M, int C, int R) {
  int s, rc;
  split_rule(M, C, R, &s, &rc);
  return s > 1 ? (size_t)s * M * C : 0;
}

int launch(const float* A, long sam, long sar, const float* B, long sbr, long sbc, int M, int C, int R, bool may_split,
           float* part, const Epi& epi, hipStream_t stream) {
  int splits = 1, rchunk = cdiv(R, KT) * KT;
  if (may_split) split_rule(M, C, R, &splits, &rchunk);
  const dim3 grid(cdiv(C, TN), cdiv(M, TM), splits);
  hipLaunchKernelGGL(gemm_f32_kernel, grid, 256, 0, stream, A, sam, sar, B, sbr, sbc, M, C, R, rchunk,
                     splits > 1 ? part : (float*)nullptr, epi);
  if (splits > 1) {
    const size_t MC = (size_t)M * C;
    hipLaunchKernelGGL(split_reduce_kernel, (unsigned)((MC + 255) / 256), 256, 0, stream, part, splits, M, C, epi);
  }
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

}  // namespace

extern "C" {

int es_dense_wide_tile(int which) { return which == 0 ? TM : which == 1 ? TN : which == 2 ? KT : TARGET_WG; }

int es_dense_wide_fwd(const float* X, int ldx, const float* W, const float* b, float* Y, int ldy, int n, int K, int N,
                      int act, float slope, const void* keep, float keep_scale, hipStream_t stream) {
  if (n <= 0 || n > MAXROWS || K <= 0 || N <= 0 || K > MAXD || N > MAXD || act < 0 || act > 2 || ldx < K || ldy < N)
    return ES_BAD_SHAPE;
  if (!X || !W || !Y) return ES_BAD_ARG;
  const Epi epi{MODE_FWD, Y, ldy, b, act, slope, (const uint8_t*)keep, keep_scale, 0};
  return launch(X, ldx, 1, W, 1, K, n, N, K, false, nullptr, epi, stream);
}

// floats: dpre [n, N], then the larger of the two products' split partials (dX's only with want_dx)
size_t es_dense_wide_bwd_workspace(int n, int K, int N, int want_dx) {
  if (n <= 0 || n > MAXROWS || K <= 0 || N <= 0 || K > MAXD || N > MAXD) return 0;
  const size_t dw = partial_floats(N, K, n), dx = want_dx ? partial_floats(n, K, N) : 0;
  return (size_t)n * N + std::max(dw, dx);
}

int es_dense_wide_bwd(const float* dY, int lddy, const float* Yact, int ldya, int act, float slope, const void* keep,
                      float keep_scale, const float* X, int ldx, const float* W, float* dX, int lddx,
                      int accumulate_dx, float* dW, float* db, int n, int K, int N, float* workspace,
                      hipStream_t stream) {
  if (n <= 0 || n > MAXROWS || K <= 0 || N <= 0 || K > MAXD || N > MAXD || act < 0 || act > 2) return ES_BAD_SHAPE;
  if (lddy < N || ldx < K || (act && ldya < N) || (dX && lddx < K)) return ES_BAD_SHAPE;
  if (!dY || !X || !W || !dW || !workspace || (act && !Yact)) return ES_BAD_ARG;
  float* dpre = workspace;
  float* part = workspace + (size_t)n * N;
  const size_t nN = (size_t)n * N;
  hipLaunchKernelGGL(dpre_kernel, (unsigned)((nN + 255) / 256), 256, 0, stream, dY, lddy, Yact, ldya, act, slope,
                     (const uint8_t*)keep, keep_scale, dpre, n, N);
  if (db) hipLaunchKernelGGL(colsum_kernel, (unsigned)((N + 63) / 64), 256, 0, stream, dpre, db, n, N);
  // dW[c][k] = sum_i dpre[i][c] X[i][k]
  const Epi ew{MODE_DW, dW, K, nullptr, 0, 0.f, nullptr, 1.f, 0};
  int rc = launch(dpre, 1, N, X, ldx, 1, N, K, n, true, part, ew, stream);
  if (rc != ES_OK || !dX) return rc;
  // dX[i][k] (+)= sum_c dpre[i][c] W[c][k] (the partials' region is free again: same stream)
  const Epi ex{MODE_DX, dX, lddx, nullptr, 0, 0.f, nullptr, 1.f, accumulate_dx};
  return launch(dpre, N, 1, W, K, 1, n, K, N, true, part, ex, stream);
}

}  // extern "C"
