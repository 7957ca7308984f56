// g2o's Levenberg-Marquardt control (optimization_algorithm_levenberg.cpp:61-189,
// sparse_optimizer_terminate_action.cpp:21-72), one definition for the device-driven loop
// (k_edges_end's last workgroup), the host-driven loop (Optimizer::run) and the replay hooks that
// pin it to the reference text (tests/test_g2o_golden.py).  No HIP include: __host__ __device__
// under hipcc, inline under a host compiler.  Needs -ffp-contract=off (cube_rn).
#pragma once
#include "../../include/mcs_ba.h"

#if defined(__HIPCC__)
#define MCS_LM_FN __host__ __device__ inline
#else
#define MCS_LM_FN inline
#endif

namespace mcs {
namespace ba {

// Device-driven, the block lives in device memory and k_edges_end updates it after every trial,
// so the host enqueues trial after trial without reading anything back: kernels of a step that
// is no longer needed (done) return at once; the linearisation of a step runs only when the
// previous trial ended an iteration (lin).  Host-driven, it is a local of Optimizer::run.
constexpr int kLmTraceCap = 64;
struct LmCtl {
  double lambda, currentChi, iniChi, lastChi, tau, gain_threshold;
  double chi0, lambda_final;
  int ni, qmax, nBad, it, iter;
  int done, lin, restore, stop_out, ext_stop;
  int dev_err;       // a solve's hand-off wait timed out (ldlt::kFlagTimeout): the run is aborted
  int spec_lin;      // k_edges_end linearises every trial into the other Jacobian buffer
  int jbuf;          // the linearisation buffer of the current iteration (0 / 1)
  int max_iterations, max_trials, terminate_max_iter;
  unsigned arrive;   // k_edges_end's arrival counter (0 between launches)
  double trace[kLmTraceCap];   // chi2 per iteration (the device path's carrier)
};

// a zeroed block with the options in place, before the first linearisation; done, spec_lin and
// jbuf are the caller's
MCS_LM_FN void lm_init(LmCtl& c, const mcs_ba_options& o) {
  c = LmCtl{};
  c.tau = o.tau; c.gain_threshold = o.gain_threshold;
  c.max_iterations = o.max_iterations; c.max_trials = o.max_trials;
  c.terminate_max_iter = o.terminate_max_iter;
  c.lin = 1; c.ni = 2;
}

// x^3 rounded once (double-double product), the value std::pow(x, 3) returns: host and device
// (and every rank) take the identical lambda step
MCS_LM_FN double cube_rn(double x) {
  const double p = x * x;
  const double pe = __builtin_fma(x, x, -p);       // x^2 = p + pe exactly
  const double h = p * x;
  // overflow: pow(x, 3) returns +-inf (the error terms would turn it into NaN, and the LM's
  // alpha = 1 - pow(2 rho - 1, 3) must become -inf so that lambda *= 1/3; g2o_solver.npz
  // scenario 27 has such a step)
  if (!__builtin_isfinite(h)) return h;
  const double he = __builtin_fma(p, x, -h);       // p x = h + he exactly
  return h + (he + pe * x);
}

// chi2 of the starting point -> currentChi (the optimize() call's activeRobustChi2)
MCS_LM_FN void lm_start_body(LmCtl* c, double chi) {
  c->chi0 = chi;
  c->currentChi = chi;
  c->iniChi = chi;
}
// lambda of iteration 0: tau * max diagonal (computeLambdaInit,
// optimization_algorithm_levenberg.cpp:166-180); pt / pose = max |diagonal| of Hll / Hpp
MCS_LM_FN void lm_lambda0_body(LmCtl* c, double pt, double pose) {
  c->lambda = c->tau * __builtin_fmax(pt, pose);
  c->ni = 2;
  c->nBad = 0;
}

// After a trial (one thread): OptimizationAlgorithmLevenberg::solve's accept / reject (:99-163)
// and, when the iteration ends, Raul's nBad stop and the terminate action
// (sparse_optimizer_terminate_action.cpp:43-72).  sc = {robust chi2, points' model decrease,
// poses' model decrease}; zero_pivot / timeout = the solve's ldlt:: status bits, tested by the
// caller; stop = the caller's stop flag as every rank sees it.  Afterwards: restore = pop the
// trial's state, lin = linearise before the next trial, done = the run has ended, dev_err =
// report the timeout.
MCS_LM_FN void lm_step(LmCtl* c, const double sc[3], bool zero_pivot, bool timeout, int stop) {
  c->ext_stop = stop;
  if (timeout) {        // x is garbage: no LM decision, the host reports MCS_ERR_HIP
    c->dev_err = 1;
    c->done = 1;
    c->restore = 1;     // k_edges_end pops the trial's state
    return;
  }
  double tempChi = sc[0];
  if (zero_pivot) tempChi = 1.7976931348623157e308;
  double rho = c->currentChi - tempChi;
  double scale = sc[2] + sc[1];
  scale += 1e-3;
  rho /= scale;
  if (rho > 0 && __builtin_isfinite(tempChi)) {
    // (the reference's std::min / std::max differ from fmin / fmax only for a NaN alpha, which
    // cannot reach these lines: rho > 0 and a finite tempChi exclude it)
    double alpha = 1. - cube_rn(2 * rho - 1);
    alpha = __builtin_fmin(alpha, 2. / 3.);
    c->lambda *= __builtin_fmax(1. / 3., alpha);
    c->ni = 2;
    c->currentChi = tempChi;
    c->restore = 0;
    if (c->spec_lin) c->jbuf ^= 1;   // the trial's linearisation (k_edges_end) is current
  } else {
    c->lambda *= c->ni;
    c->ni *= 2;
    c->restore = 1;   // the state is popped right after this decision
  }
  c->qmax++;
  if (rho < 0 && c->qmax < c->max_trials && !stop) {
    c->lin = 0;       // the next step retries the trial with the larger lambda
  } else {
    int result = 0;
    if (c->qmax == c->max_trials || rho == 0) result = 1;
    else {
      if ((c->iniChi - c->currentChi) * 1e3 < c->iniChi) c->nBad++;
      else c->nBad = 0;
      if (c->nBad >= 3) result = 1;
    }
    c->it++;
    const int i = c->iter;
    const double cur = c->currentChi;
    if (i < kLmTraceCap) c->trace[i] = cur;
    int stopOpt = 0;
    if (i == 0) c->lastChi = cur;
    else {
      if (i < c->terminate_max_iter) {
        const double gain = (c->lastChi - cur) / cur;
        c->lastChi = cur;
        if (gain >= 0 && gain < c->gain_threshold) stopOpt = 1;
      } else {
        stopOpt = 1;
      }
    }
    if (stopOpt) c->stop_out = 1;
    c->lambda_final = c->lambda;
    c->iter = i + 1;
    if (c->iter >= c->max_iterations || stop || stopOpt || result != 0) {
      c->done = 1;
    } else {
      c->lin = 1;
      c->qmax = 0;
      c->iniChi = c->currentChi;
    }
  }
}

}  // namespace ba
}  // namespace mcs
