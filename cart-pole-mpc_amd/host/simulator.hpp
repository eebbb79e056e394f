// simulator.hpp -- pendulum::Simulator with the reference's signatures
// (optimization/simulator.hpp:10-29); the integration runs in libcpmpc.so's sim kernel (fp64).
#pragma once
#include <array>

#include "structs.hpp"

namespace pendulum {

// Encapsulates the system state and integrates it forward in time.
class Simulator {
 public:
  // Step the simulator forward by `dt` with control input `u` (simulator.cc:11-23).
  // Throws std::invalid_argument for dt < 0 or non-finite u (simulator.cc:13-14).
  void Step(const SingleCartPoleParams& params, double dt, double u, const Vector2& f_base,
            const Vector2& f_mass);

  SingleCartPoleState GetState() const noexcept {
    return SingleCartPoleState{state_[0], state_[1], state_[2], state_[3]};
  }

  void SetState(const SingleCartPoleState& state) noexcept { state_ = state.ToVector(); }

  // The first derivatives of the map Step applies, at the current state (which is not changed): A = dx+/dx row-major
  // [4][4] and B = dx+/du [4], the control held over dt -- the product of the sub-steps' RK4 Jacobians, the wrap of the pole
  // angle with unit derivative (include/cpmpc.h: cpmpc_sim_step_jac_batch).  Not differentiated here: params
  // (StepParamJacobian below), the forces, dt.
  // Throws as Step.
  struct StepJacobians {
    std::array<double, 16> A;
    std::array<double, 4> B;
  };
  [[nodiscard]] StepJacobians StepJacobian(const SingleCartPoleParams& params, double dt, double u, const Vector2& f_base,
                                           const Vector2& f_mass) const;

  // The derivative of the same map in the dynamics parameters, at the current state (which is not changed): P = dx+/dp
  // row-major [4][9], p in the order of SingleCartPoleParams::ToArray() {m_b, m_1, l_1, g, mu_b, v_mu_b, c_d_1, x_s, k_s},
  // and the state after the step (include/cpmpc.h: cpmpc_sim_step_param_jac_batch).  Throws as Step.
  struct StepParamJacobians {
    std::array<double, 36> P;
    std::array<double, 4> x_new;
  };
  [[nodiscard]] StepParamJacobians StepParamJacobian(const SingleCartPoleParams& params, double dt, double u,
                                                     const Vector2& f_base, const Vector2& f_mass) const;

 private:
  std::array<double, 4> state_{0.0, -3.14159265358979323846 / 2, 0.0, 0.0};  // simulator.hpp:28
};

}  // namespace pendulum
