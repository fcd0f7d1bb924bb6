// smx_schedule.hip -- step-dependent weights (smx_set_schedule): the KL weight and the learning rate as functions of the step, evaluated
// on the host in double and rounded once to float.  Each train_steps call's (beta, lr) table goes to the device beside its row ids
// (smx_step.hip: upload_order); step_begin and the optimiser's closing workgroup copy a step's entry into its StepState.
// sisua_amd/interpolation.py is the same evaluator in Python, operation for operation.
#include <math.h>

#include <algorithm>

#include "smx_model.h"

#pragma clang fp contract(off)   // (the Python evaluator rounds every operation: no fused multiply-adds here either)

namespace smx {

static const char* kSchedBuilt = "built: const, linear, power, cosine (interpolation); ExponentialDecay, InverseTimeDecay, "
                                 "PiecewiseConstantDecay, PolynomialDecay, CosineDecay (tf.keras)";

int sched_check(int32_t kind, const double* p, int32_t n) {
  SMX_REQUIRE(n >= 0 && (n == 0 || p), "schedule: null parameters");
  for (int i = 0; i < n; ++i) SMX_REQUIRE(std::isfinite(p[i]), "schedule: parameters must be finite");
  switch (kind) {
    case SMX_SCHED_CONST: SMX_REQUIRE(n == 1, "schedule const: one parameter (vmax)"); return SMX_OK;
    case SMX_SCHED_LINEAR: case SMX_SCHED_COSINE: case SMX_SCHED_POWER:
      SMX_REQUIRE(n == (kind == SMX_SCHED_POWER ? 7 : 6), "schedule interpolation: vmin, vmax, norm, cyclical, delayIn, delayOut (power: + power)");
      SMX_REQUIRE(p[2] > 0, "schedule interpolation: norm must be > 0");
      SMX_REQUIRE(p[4] >= 0 && p[5] >= 0, "schedule interpolation: delays must be >= 0");
      return SMX_OK;
    case SMX_SCHED_EXP_DECAY: case SMX_SCHED_INVTIME_DECAY:
      SMX_REQUIRE(n == 4, "schedule decay: initial_learning_rate, decay_steps, decay_rate, staircase");
      SMX_REQUIRE(p[1] > 0, "schedule decay: decay_steps must be > 0");
      return SMX_OK;
    case SMX_SCHED_PIECEWISE: {
      SMX_REQUIRE(n >= 1 && n % 2 == 1, "schedule piecewise: boundaries[k] then values[k + 1]");
      const int k = (n - 1) / 2;
      for (int i = 1; i < k; ++i) SMX_REQUIRE(p[i] > p[i - 1], "schedule piecewise: boundaries must increase");
      return SMX_OK;
    }
    case SMX_SCHED_POLY_DECAY:
      SMX_REQUIRE(n == 5, "schedule polynomial: initial_learning_rate, decay_steps, end_learning_rate, power, cycle");
      SMX_REQUIRE(p[1] > 0, "schedule polynomial: decay_steps must be > 0");
      return SMX_OK;
    case SMX_SCHED_COSINE_DECAY:
      SMX_REQUIRE(n == 3, "schedule cosine decay: initial_learning_rate, decay_steps, alpha");
      SMX_REQUIRE(p[1] > 0, "schedule cosine decay: decay_steps must be > 0");
      return SMX_OK;
    default: break;
  }
  set_error(std::string("schedule: unknown kind; ") + kSchedBuilt);
  return SMX_ERR_INVALID;
}

// the value at `step` (>= 0) of a checked schedule
double sched_value(int32_t kind, const double* p, int32_t n, double step) {
  switch (kind) {
    case SMX_SCHED_CONST: return p[0];
    case SMX_SCHED_LINEAR: case SMX_SCHED_POWER: case SMX_SCHED_COSINE: {
      const double vmin = p[0], vmax = p[1], norm = p[2], din = p[4], dout = p[5];
      const double x = p[3] != 0.0 ? fmod(step, din + norm + dout) : step;
      if (x < din) return vmin;
      const double a = (x - din) / norm;
      if (a >= 1.0) return vmax;   // (the ramp's ends are the end points themselves, no arithmetic on them)
      if (a == 0.0) return vmin;
      const double f = kind == SMX_SCHED_LINEAR ? a : kind == SMX_SCHED_POWER ? pow(a, p[6]) : 0.5 - 0.5 * cos(M_PI * a);
      return vmin + (vmax - vmin) * f;
    }
    case SMX_SCHED_EXP_DECAY: case SMX_SCHED_INVTIME_DECAY: {
      double q = step / p[1];
      if (p[3] != 0.0) q = floor(q);
      return kind == SMX_SCHED_EXP_DECAY ? p[0] * pow(p[2], q) : p[0] / (1.0 + p[2] * q);
    }
    case SMX_SCHED_PIECEWISE: {
      const int k = (n - 1) / 2;
      for (int i = 0; i < k; ++i)
        if (step <= p[i]) return p[k + i];
      return p[2 * k];
    }
    case SMX_SCHED_POLY_DECAY: {
      double s = step, ds = p[1];
      if (p[4] != 0.0) ds = ds * (s == 0.0 ? 1.0 : ceil(s / ds));
      else s = std::min(s, ds);
      return (p[0] - p[2]) * pow(1.0 - s / ds, p[3]) + p[2];
    }
    case SMX_SCHED_COSINE_DECAY: {
      const double s = std::min(step, p[1]);
      const double c = 0.5 * (1.0 + cos(M_PI * (s / p[1])));
      return p[0] * ((1.0 - p[2]) * c + p[2]);
    }
    default: return 0.0;
  }
}

static double sched_at(const smx_model* m, int target, double step) {
  const std::vector<double>& p = m->sched_p[target];
  if (p.empty()) return (double)(target == SMX_SCHED_BETA ? m->cfg.beta : m->cfg.lr);
  return sched_value(m->sched_kind[target], p.data(), (int32_t)p.size(), step);
}

float sched_beta(const smx_model* m, uint32_t step) { return (float)sched_at(m, SMX_SCHED_BETA, (double)step); }

// (beta, lr) of the n_steps steps from the model's step on; the learning rate is keyed by the rule's own count step - t0
void sched_fill(const smx_model* m, float* dst, size_t n_steps) {
  for (size_t i = 0; i < n_steps; ++i) {
    const uint32_t step = m->h_next + (uint32_t)i;
    dst[2 * i] = (float)sched_at(m, SMX_SCHED_BETA, (double)step);
    dst[2 * i + 1] = (float)sched_at(m, SMX_SCHED_LR, (double)(step >= m->opt_t0 ? step - m->opt_t0 : 0u));
  }
}

}  // namespace smx

extern "C" {

int smx_set_schedule(smx_model* m, int32_t target, int32_t kind, const double* params, int32_t n) {
  SMX_REQUIRE(m, "null model");
  SMX_REQUIRE(target == SMX_SCHED_BETA || target == SMX_SCHED_LR, "schedule: target must be SMX_SCHED_BETA or SMX_SCHED_LR");
  SMX_CHECK(smx::sched_check(kind, params, n));
  m->sched_kind[target] = kind;
  m->sched_p[target].assign(params, params + n);
  return SMX_OK;
}

int smx_get_schedule(const smx_model* m, int32_t target, int32_t* kind, double* params, int32_t cap, int32_t* n) {
  SMX_REQUIRE(m, "null model");
  SMX_REQUIRE(target == SMX_SCHED_BETA || target == SMX_SCHED_LR, "schedule: target must be SMX_SCHED_BETA or SMX_SCHED_LR");
  std::vector<double> p = m->sched_p[target];
  int32_t k = m->sched_kind[target];
  if (p.empty()) { k = SMX_SCHED_CONST; p.assign(1, (double)(target == SMX_SCHED_BETA ? m->cfg.beta : m->cfg.lr)); }
  if (kind) *kind = k;
  if (params) for (int32_t i = 0; i < cap && i < (int32_t)p.size(); ++i) params[i] = p[i];
  if (n) *n = (int32_t)p.size();
  return SMX_OK;
}

int smx_schedule_eval(int32_t kind, const double* params, int32_t n, int64_t first_step, int32_t count, float* out) {
  SMX_REQUIRE(first_step >= 0 && count >= 0 && (count == 0 || out), "schedule eval: bad range");
  SMX_CHECK(smx::sched_check(kind, params, n));
  for (int32_t i = 0; i < count; ++i) out[i] = (float)smx::sched_value(kind, params, n, (double)(first_step + i));
  return SMX_OK;
}

}  // extern "C"
