#pragma once
// smx_act.h -- hidden-layer activations of NetConf(activation=...) and their derivatives (smx_set_activation).
// act_fwd(kind, y) is the activation of a pre-activation y; act_grad(kind, h) its derivative, written in terms of the
// activation's own output h = act_fwd(kind, y) (the form the backward launches and the float64 reference use).  Plain libm
// exp / expm1 / log1p / tanh (not the fast intrinsics): these values feed gradients compared at 1e-4.
// ReLU (SMX_ACT_RELU) never comes here: its launches keep their own max(y, 0) + leak min(y, 0) code (the GEN_ACT = false forms).
#include <hip/hip_runtime.h>
#include "../../include/sisua_hip.h"

namespace smx {

constexpr float ACT_LEAKY_SLOPE = 0.2f;                   // [3P-recall] tf.nn.leaky_relu's default alpha
constexpr float ACT_SELU_LAMBDA = 1.0507009873554805f;    // [3P-recall] the Keras / Klambauer et al. SELU constants
constexpr float ACT_SELU_ALPHA = 1.6732632423543772f;

__device__ inline float act_fwd(int kind, float y) {
  switch (kind) {
    case SMX_ACT_LINEAR: return y;
    case SMX_ACT_LEAKY_RELU: return y > 0.f ? y : ACT_LEAKY_SLOPE * y;
    case SMX_ACT_ELU: return y > 0.f ? y : expm1f(y);
    case SMX_ACT_SELU: return y > 0.f ? ACT_SELU_LAMBDA * y : (ACT_SELU_LAMBDA * ACT_SELU_ALPHA) * expm1f(y);
    case SMX_ACT_TANH: return tanhf(y);
    case SMX_ACT_SIGMOID: {   // (one exp(-|y|): no overflow at either end)
      const float e = expf(-fabsf(y));
      const float inv = 1.f / (1.f + e);
      return y >= 0.f ? inv : e * inv;
    }
    case SMX_ACT_SOFTPLUS: return fmaxf(y, 0.f) + log1pf(expf(-fabsf(y)));
    default: return fmaxf(y, 0.f);
  }
}

__device__ inline float act_grad(int kind, float h) {
  switch (kind) {
    case SMX_ACT_LINEAR: return 1.f;
    case SMX_ACT_LEAKY_RELU: return h > 0.f ? 1.f : ACT_LEAKY_SLOPE;
    case SMX_ACT_ELU: return h > 0.f ? 1.f : h + 1.f;
    case SMX_ACT_SELU: return h > 0.f ? ACT_SELU_LAMBDA : h + ACT_SELU_LAMBDA * ACT_SELU_ALPHA;
    case SMX_ACT_TANH: return (1.f - h) * (1.f + h);
    case SMX_ACT_SIGMOID: return h * (1.f - h);
    case SMX_ACT_SOFTPLUS: return -expm1f(-h);   // sigmoid(y) = 1 - exp(-softplus(y))
    default: return h > 0.f ? 1.f : 0.f;
  }
}

}  // namespace smx
