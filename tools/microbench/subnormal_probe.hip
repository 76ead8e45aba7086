// Do v_dot2_f32_f16 and v_mfma_f32_16x16x32_f16 keep fp16 subnormal operands on gfx950, and is their fp32 result the same bits when
// the operands are moved by exact powers of two?  (`make -C tools/microbench subnormal_probe`; stand-alone, no library.)
//
// One instruction per result on random operands: the "layer" has one operand at N(0,1) * 2^shift (rounded into fp16 first), the
// other at N(0,1) * 2^6 and C at 2^(shift + 6); the "twin" is the same numbers moved exactly to unit magnitude; a third run has
// the layer's fp16 subnormals set to zero (what a flushing unit would compute with).  Per line: the share of subnormals in the
// small operand, how many fp32 results differ in their bits from the twin's (after the exact move back), how many equal the
// flushed run, and the mean-relative distance of layer and twin from the fp64 sum and of the layer from the fp64 sum of the
// flushed operands.  Measured on the MI355X ("Magnitudes"): nothing is flushed (layer and twin within
// 4e-8 of the fp64 sum, 0.36 - 0.45 from the flushed one); at shift -14 (68 % subnormal) 5 - 6 % of the MFMA results and 1 - 2 %
// of the dot2 results differ from the twin's in their last bits, whichever MFMA operand is the small one; at -10 none (MFMA) / a
// dozen of 65536 (dot2); at -8 none.  tests/test_magnitude_gpu.py rests its five expected failures on this.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

__global__ void mfma_k(const _Float16* A, const _Float16* B, const float* C, float* D) {
  const int l = threadIdx.x, t = blockIdx.x;
  f16x8 a, b;
  for (int i = 0; i < 8; ++i) { a[i] = A[(t * 64 + l) * 8 + i]; b[i] = B[(t * 64 + l) * 8 + i]; }
  f32x4 c;
  for (int j = 0; j < 4; ++j) c[j] = C[(t * 64 + l) * 4 + j];
  f32x4 d = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  for (int j = 0; j < 4; ++j) D[(t * 64 + l) * 4 + j] = d[j];
}

__global__ void dot2_k(const _Float16* A, const _Float16* B, const float* C, float* D, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    f16x2 a = {A[2 * i], A[2 * i + 1]}, b = {B[2 * i], B[2 * i + 1]};
    D[i] = __builtin_amdgcn_fdot2(a, b, C[i], false);
  }
}

static const int T = 256;  // tiles
static bool is_sub(_Float16 h) { float f = std::fabs((float)h); return f > 0 && f < 0x1p-14f; }

struct Set { std::vector<_Float16> A, B; std::vector<float> C; };

static int run_mfma(const Set& s, std::vector<float>& D) {
  _Float16 *dA, *dB; float *dC, *dD;
  size_t nA = s.A.size() * 2, nC = s.C.size() * 4;
  CK(hipMalloc(&dA, nA)); CK(hipMalloc(&dB, nA)); CK(hipMalloc(&dC, nC)); CK(hipMalloc(&dD, nC));
  CK(hipMemcpy(dA, s.A.data(), nA, hipMemcpyHostToDevice)); CK(hipMemcpy(dB, s.B.data(), nA, hipMemcpyHostToDevice));
  CK(hipMemcpy(dC, s.C.data(), nC, hipMemcpyHostToDevice));
  mfma_k<<<T, 64>>>(dA, dB, dC, dD);
  CK(hipDeviceSynchronize());
  D.resize(s.C.size());
  CK(hipMemcpy(D.data(), dD, nC, hipMemcpyDeviceToHost));
  CK(hipFree(dA)); CK(hipFree(dB)); CK(hipFree(dC)); CK(hipFree(dD));
  return 0;
}

static int run_dot2(const Set& s, std::vector<float>& D) {
  _Float16 *dA, *dB; float *dC, *dD;
  const int n = (int)s.C.size();
  CK(hipMalloc(&dA, n * 4)); CK(hipMalloc(&dB, n * 4)); CK(hipMalloc(&dC, n * 4)); CK(hipMalloc(&dD, n * 4));
  CK(hipMemcpy(dA, s.A.data(), n * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dB, s.B.data(), n * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dC, s.C.data(), n * 4, hipMemcpyHostToDevice));
  dot2_k<<<(n + 255) / 256, 256>>>(dA, dB, dC, dD, n);
  CK(hipDeviceSynchronize());
  D.resize(n);
  CK(hipMemcpy(D.data(), dD, n * 4, hipMemcpyDeviceToHost));
  CK(hipFree(dA)); CK(hipFree(dB)); CK(hipFree(dC)); CK(hipFree(dD));
  return 0;
}

// fp64 reference of the mfma tile: A lane l -> row l % 16, k = (l / 16) * 8 + i; B lane l -> col l % 16, same k; D lane l -> col l % 16, row (l / 16) * 4 + j
static void ref_mfma(const Set& s, std::vector<double>& R) {
  R.assign(s.C.size(), 0.0);
  for (int t = 0; t < T; ++t)
    for (int l = 0; l < 64; ++l)
      for (int j = 0; j < 4; ++j) {
        const int col = l % 16, row = (l / 16) * 4 + j;
        double acc = s.C[(t * 64 + l) * 4 + j];
        for (int k = 0; k < 32; ++k) {
          const int la = (k / 8) * 16 + row, lb = (k / 8) * 16 + col;
          acc += (double)(float)s.A[(t * 64 + la) * 8 + k % 8] * (double)(float)s.B[(t * 64 + lb) * 8 + k % 8];
        }
        R[(t * 64 + l) * 4 + j] = acc;
      }
}

static void ref_dot2(const Set& s, std::vector<double>& R) {
  R.resize(s.C.size());
  for (size_t i = 0; i < s.C.size(); ++i)
    R[i] = (double)s.C[i] + (double)(float)s.A[2 * i] * (double)(float)s.B[2 * i] + (double)(float)s.A[2 * i + 1] * (double)(float)s.B[2 * i + 1];
}

// base N(0,1) values; layer: sub operand at 2^-14 (rounded), other at 2^6, C at 2^-8; twin: everything moved to unit magnitude exactly
static void build(int n16, int nC, bool sub_is_A, int sub_shift, bool with_c, unsigned seed, Set& layer, Set& twin, Set& flushed, double& share) {
  std::mt19937 g(seed);
  std::normal_distribution<float> N(0.f, 1.f);
  layer.A.resize(n16); layer.B.resize(n16); layer.C.resize(nC);
  twin = layer; flushed = layer;
  long nsub = 0;
  for (int i = 0; i < n16; ++i) {
    _Float16 lo = (_Float16)std::ldexp(N(g), sub_shift);          // low side first
    _Float16 hi = (_Float16)std::ldexp((float)lo, -sub_shift);   // exact up-shift
    _Float16 o = (_Float16)N(g);
    _Float16 o_up = (_Float16)std::ldexp((float)o, 6);
    nsub += is_sub(lo);
    _Float16 fl = is_sub(lo) ? (_Float16)0.f : lo;
    (sub_is_A ? layer.A : layer.B)[i] = lo; (sub_is_A ? layer.B : layer.A)[i] = o_up;
    (sub_is_A ? twin.A : twin.B)[i] = hi;   (sub_is_A ? twin.B : twin.A)[i] = o;
    (sub_is_A ? flushed.A : flushed.B)[i] = fl; (sub_is_A ? flushed.B : flushed.A)[i] = o_up;
  }
  for (int i = 0; i < nC; ++i) {
    float c = with_c ? 4.f * N(g) : 0.f;
    twin.C[i] = c; layer.C[i] = flushed.C[i] = std::ldexp(c, sub_shift + 6);
  }
  share = (double)nsub / n16;
}

static void report(const char* what, int shift, const std::vector<float>& D, const std::vector<float>& Dt, const std::vector<float>& Df,
                   const std::vector<double>& R, const std::vector<double>& Rf, double share) {
  long differ = 0, eq_flushed = 0, max_ulp = 0;
  double err = 0, err_t = 0, err_flush_ref = 0, mean = 0;
  for (size_t i = 0; i < D.size(); ++i) {
    const float up = std::ldexp(D[i], -(shift + 6));  // exact
    int32_t a, b; std::memcpy(&a, &up, 4); std::memcpy(&b, &Dt[i], 4);
    if (a != b) { ++differ; long d = std::labs((long)a - (long)b); if (d > max_ulp) max_ulp = d; }
    eq_flushed += D[i] == Df[i];
    err += std::fabs(D[i] - R[i]); err_t += std::fabs(std::ldexp((double)Dt[i], shift + 6) - R[i]); err_flush_ref += std::fabs(D[i] - Rf[i]); mean += std::fabs(R[i]);
  }
  printf("%-44s sub share %.2f | differ from twin %ld of %zu (max %ld ulp32) | equal to flushed run %ld | mean-rel vs fp64: layer %.3e twin %.3e, layer vs flushed-fp64 %.3e\n",
         what, share, differ, D.size(), max_ulp, eq_flushed, err / mean, err_t / mean, err_flush_ref / mean);
}

int main() {
  for (int shift : {-14, -10, -8}) {       // -14: 68 % subnormal; -10: a few; -8: control, (almost) none
    for (int sub_is_A = 0; sub_is_A < 2; ++sub_is_A)
      for (int with_c = 0; with_c < 2; ++with_c) {
        Set L, Tw, F; double share;
        build(T * 64 * 8, T * 64 * 4, sub_is_A, shift, with_c, 7 + shift + 2 * sub_is_A + with_c, L, Tw, F, share);
        std::vector<float> D, Dt, Df; std::vector<double> R, Rf;
        if (run_mfma(L, D) || run_mfma(Tw, Dt) || run_mfma(F, Df)) return 2;
        ref_mfma(L, R); ref_mfma(F, Rf);
        char what[96]; snprintf(what, sizeof what, "mfma16x16x32f16 shift %d small=%s C=%d", shift, sub_is_A ? "A" : "B", with_c);
        report(what, shift, D, Dt, Df, R, Rf, share);
      }
    for (int with_c = 0; with_c < 2; ++with_c) {
      Set L, Tw, F; double share; const int n = 1 << 16;
      build(2 * n, n, true, shift, with_c, 99 + shift + with_c, L, Tw, F, share);
      std::vector<float> D, Dt, Df; std::vector<double> R, Rf;
      if (run_dot2(L, D) || run_dot2(Tw, Dt) || run_dot2(F, Df)) return 2;
      ref_dot2(L, R); ref_dot2(F, Rf);
      char what[96]; snprintf(what, sizeof what, "dot2_f32_f16 shift %d C=%d", shift, with_c);
      report(what, shift, D, Dt, Df, R, Rf, share);
    }
  }
  return 0;
}
