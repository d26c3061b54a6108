// Host-only check of the wide dense entry points' argument validation (es_dense_wide_fwd, es_dense_wide_bwd,
// es_dense_wide_bwd_workspace): every call below must be refused with -1 (bad shape) or -2 (bad argument), or
// answer 0 floats, before any launch, so the program needs no GPU and the pointers are never followed.
// Built against csrc/dense_wide.hip itself with the host side under AddressSanitizer + UBSan:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       -I endoscopy-image-classification_amd/csrc -I include \
//       scripts/dense_wide_args_check.cpp endoscopy-image-classification_amd/csrc/dense_wide.hip \
//       -o dense_wide_args_check
//   ./dense_wide_args_check
#include <cstdint>
#include <cstdio>

#include "endossl.h"

namespace {

int failures = 0;

void expect(const char* what, long rc, long want) {
  if (rc != want) {
    std::printf("FAIL %-44s returned %ld, expected %ld\n", what, rc, want);
    ++failures;
  } else {
    std::printf("ok   %-44s -> %ld\n", what, rc);
  }
}

// never dereferenced: a refusal returns before any launch
float* const P = reinterpret_cast<float*>(uintptr_t{0x1000});

struct Fwd {
  const float* X = P;
  int ldx = 8;
  const float* W = P;
  float* Y = P;
  int ldy = 6;
  int n = 4, K = 8, N = 6, act = 1;
};

int run(const Fwd& a) {
  return es_dense_wide_fwd(a.X, a.ldx, a.W, P, a.Y, a.ldy, a.n, a.K, a.N, a.act, 0.1f, nullptr, 1.f, nullptr);
}

struct Bwd {
  const float* dY = P;
  int lddy = 6;
  const float* Yact = P;
  int ldya = 6;
  int act = 1;
  const float* X = P;
  int ldx = 8;
  const float* W = P;
  float* dX = P;
  int lddx = 8;
  float* dW = P;
  int n = 4, K = 8, N = 6;
  float* ws = P;
};

int run(const Bwd& a) {
  return es_dense_wide_bwd(a.dY, a.lddy, a.Yact, a.ldya, a.act, 0.1f, nullptr, 1.f, a.X, a.ldx, a.W, a.dX, a.lddx, 0,
                           a.dW, P, a.n, a.K, a.N, a.ws, nullptr);
}

}  // namespace

#define FWD(WHAT, WANT, ...)   \
  {                            \
    Fwd f;                     \
    __VA_ARGS__;               \
    expect("fwd " WHAT, run(f), WANT); \
  }
#define BWD(WHAT, WANT, ...)   \
  {                            \
    Bwd b;                     \
    __VA_ARGS__;               \
    expect("bwd " WHAT, run(b), WANT); \
  }

int main() {
  FWD("n = 0", -1, f.n = 0)
  FWD("n < 0", -1, f.n = -3)
  FWD("n = 65535 * 32 + 1", -1, f.n = 65535 * 32 + 1)
  FWD("K = 0", -1, f.K = 0)
  FWD("N = 0", -1, f.N = 0)
  FWD("K = 4097", -1, f.K = 4097; f.ldx = 4097)
  FWD("N = 4097", -1, f.N = 4097; f.ldy = 4097)
  FWD("act = 3", -1, f.act = 3)
  FWD("act = -1", -1, f.act = -1)
  FWD("ldx < K", -1, f.ldx = 7)
  FWD("ldy < N", -1, f.ldy = 5)
  FWD("X null", -2, f.X = nullptr)
  FWD("W null", -2, f.W = nullptr)
  FWD("Y null", -2, f.Y = nullptr)
  BWD("n = 0", -1, b.n = 0)
  BWD("n = 65535 * 32 + 1", -1, b.n = 65535 * 32 + 1)
  BWD("K = 0", -1, b.K = 0)
  BWD("N = 0", -1, b.N = 0)
  BWD("K = 4097", -1, b.K = 4097; b.ldx = b.lddx = 4097)
  BWD("N = 4097", -1, b.N = 4097; b.lddy = b.ldya = 4097)
  BWD("act = 3", -1, b.act = 3)
  BWD("act = -1", -1, b.act = -1)
  BWD("lddy < N", -1, b.lddy = 5)
  BWD("ldya < N with an activation", -1, b.ldya = 5)
  BWD("ldx < K", -1, b.ldx = 7)
  BWD("lddx < K with dX", -1, b.lddx = 7)
  BWD("dY null", -2, b.dY = nullptr)
  BWD("Yact null with an activation", -2, b.Yact = nullptr)
  BWD("X null", -2, b.X = nullptr)
  BWD("W null", -2, b.W = nullptr)
  BWD("dW null", -2, b.dW = nullptr)
  BWD("workspace null", -2, b.ws = nullptr)
  expect("workspace n = 0", (long)es_dense_wide_bwd_workspace(0, 8, 6, 1), 0);
  expect("workspace n = 65535 * 32 + 1", (long)es_dense_wide_bwd_workspace(65535 * 32 + 1, 8, 6, 1), 0);
  expect("workspace K = 0", (long)es_dense_wide_bwd_workspace(4, 0, 6, 1), 0);
  expect("workspace N = 0", (long)es_dense_wide_bwd_workspace(4, 8, 0, 1), 0);
  expect("workspace K = 4097", (long)es_dense_wide_bwd_workspace(4, 4097, 6, 1), 0);
  expect("workspace N = 4097", (long)es_dense_wide_bwd_workspace(4, 8, 4097, 0), 0);
  // the largest accepted sizes: dpre + the larger product's partials, no overflow on the way
  expect("workspace 4 x 8 x 6, no dX: dpre + dW's 1 split", (long)es_dense_wide_bwd_workspace(4, 8, 6, 0), 24);
  expect("workspace (1 << 20) x 4096 x 4096 fits size_t",
         (long)(es_dense_wide_bwd_workspace(1 << 20, 4096, 4096, 1) >= ((size_t)1 << 32)), 1);
  std::printf(failures ? "%d FAILED\n" : "all refused as expected\n", failures);
  return failures ? 1 : 0;
}
