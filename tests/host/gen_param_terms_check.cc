// gen_param_terms_check.cc -- the parameter partials tools/gen_dynamics.py emits for the cart + double pendulum
// (csrc/double_pendulum_param_gen.hpp: dF/dp, dM/dp with their masks) compiled FOR THE HOST: da/dp_j = M^-1 (dF/dp_j - dM/dp_j a)
// against central differences, in each parameter, of the accelerations a = M^-1 F of the generated terms
// (csrc/double_pendulum_gen.hpp).  Bound: 1e-7 of the case's largest entry.  No GPU.
// Build (tests/test_sim_param_ref.py does it): g++ -O1 -std=c++17 -I<repo> tests/host/gen_param_terms_check.cc
#include <cmath>
#include <cstdio>
#include <random>

#define __device__
#define __host__
#define __forceinline__ inline
namespace cpmpc {
template <typename R>
struct Math;
template <>
struct Math<double> {
  static void sincos(double x, double& s, double& c) {
    s = std::sin(x);
    c = std::cos(x);
  }
};
}  // namespace cpmpc
#include "cart-pole-mpc_amd/csrc/double_pendulum_gen.hpp"
#include "cart-pole-mpc_amd/csrc/double_pendulum_param_gen.hpp"

// y = M^-1 b for the symmetric positive definite 3 x 3 mass matrix (LDL^T, as the model policy does it on the device)
static void solve3(const double* M, const double* b, double* y) {
  const double d0 = M[0], L0 = M[3] / d0, L1 = M[6] / d0;
  const double d1 = M[4] - L0 * L0 * d0, L2 = (M[7] - L1 * L0 * d0) / d1;
  const double d2 = M[8] - L1 * L1 * d0 - L2 * L2 * d1;
  const double z0 = b[0], z1 = b[1] - L0 * z0, z2 = b[2] - L1 * z0 - L2 * z1;
  y[2] = z2 / d2;
  y[1] = z1 / d1 - L2 * y[2];
  y[0] = z0 / d0 - L0 * y[1] - L1 * y[2];
}

static void accel(const double* p, const double* x, double u, double* a, double* M) {
  using namespace cpmpc;
  const DoublePendulumGenConsts<double> K = double_pendulum_gen_consts<double, double>(p);
  double F[3], dF[18], dA[9], dB[9];
  double_pendulum_terms_sc<double>(K, std::sin(x[1]), std::cos(x[1]), std::sin(x[2]), std::cos(x[2]), x, u, M, F, dF, dA, dB);
  solve3(M, F, a);
}

int main() {
  using namespace cpmpc;
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  int failures = 0, cases = 0;
  double worst = 0.0;
  for (int i = 0; i < 2000; ++i) {
    double p[6] = {1.0 + 0.5 * U(rng), 0.1 + 0.05 * U(rng), 0.1 + 0.05 * U(rng), 0.25 + 0.1 * U(rng), 0.2 + 0.1 * U(rng), 9.81 + U(rng)};
    double x[6] = {U(rng), 3.2 * U(rng), 3.2 * U(rng), 2 * U(rng), 6 * U(rng), 6 * U(rng)};
    const double u = 50 * U(rng);
    double a[3], M[9];
    accel(p, x, u, a, M);
    double dFdp[18], dMdp[54];
    for (double& v : dFdp) v = 12345.0;  // masked entries must stay untouched
    for (double& v : dMdp) v = 12345.0;
    double_pendulum_param_terms_sc<double>(p, std::sin(x[1]), std::cos(x[1]), std::sin(x[2]), std::cos(x[2]), x, u, dFdp, dMdp);
    double J[3][6], Jn[3][6], scale = 0.0;
    for (int j = 0; j < 6; ++j) {
      double r[3], y[3];
      for (int r_ = 0; r_ < 3; ++r_) {
        double v = DoublePendulumParamSparsity::dFdp[r_ * 6 + j] ? dFdp[r_ * 6 + j] : 0.0;
        if (!DoublePendulumParamSparsity::dFdp[r_ * 6 + j] && dFdp[r_ * 6 + j] != 12345.0) ++failures;
        for (int k = 0; k < 3; ++k) {
          const int at = j * 9 + r_ * 3 + k;
          if (DoublePendulumParamSparsity::dMdp[at]) v -= dMdp[at] * a[k];
          else if (dMdp[at] != 12345.0) ++failures;
        }
        r[r_] = v;
      }
      solve3(M, r, y);
      const double h = 1e-5 * std::fmax(std::fabs(p[j]), 1e-3);
      double hi[6], lo[6], ah[3], al[3], Mx[9];
      for (int k = 0; k < 6; ++k) hi[k] = lo[k] = p[k];
      hi[j] += h;
      lo[j] -= h;
      accel(hi, x, u, ah, Mx);
      accel(lo, x, u, al, Mx);
      for (int r_ = 0; r_ < 3; ++r_) {
        J[r_][j] = y[r_];
        Jn[r_][j] = (ah[r_] - al[r_]) / (2 * h);
        scale = std::fmax(scale, std::fabs(Jn[r_][j]));
      }
    }
    for (int r_ = 0; r_ < 3; ++r_)
      for (int j = 0; j < 6; ++j) {
        const double e = std::fabs(J[r_][j] - Jn[r_][j]) / scale;
        worst = std::fmax(worst, e);
        if (!(e <= 1e-7) && failures++ < 20)
          std::printf("FAIL case %d da_%d/dp_%d: got %.17g, central difference %.17g (%.2e of the largest entry)\n", i, r_, j,
                      J[r_][j], Jn[r_][j], e);
      }
    ++cases;
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("OK generated parameter partials: %d double-pendulum cases, worst %.2e of the largest entry (bound 1e-7)\n", cases, worst);
  return 0;
}
