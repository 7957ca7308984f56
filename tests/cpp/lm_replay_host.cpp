// The LM controller of csrc/lm_control.hpp compiled for the host and replayed on scripted
// trials: the loop of k_lm_replay (csrc/ba_kernels.hpp), same inputs, same [n][10] output.
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC lm_replay_host.cpp -o liblm_replay_host.so
#include "../../multicol-slam-annotation_amd/csrc/lm_control.hpp"

using namespace mcs::ba;

extern "C" int lm_replay_host(const mcs_ba_options* o, const double* in, const double* trials, int n,
                              double* out) {
  LmCtl ctl;
  LmCtl* c = &ctl;
  lm_init(ctl, *o);
  c->done = o->max_iterations <= 0 ? 1 : 0;
  lm_start_body(c, in[0]);
  if (!c->done) lm_lambda0_body(c, in[1], in[2]);
  int t = 0;
  for (; t < n && !c->done; t++) {
    const double* tr = trials + 4 * t;
    const double sc[3] = {tr[0], tr[1], tr[2]};
    const double lam = c->lambda;
    lm_step(c, sc, tr[3] != 0.0, false, 0);
    double* r = out + 10 * t;
    r[0] = lam; r[1] = c->lambda; r[2] = c->ni; r[3] = c->restore ? 0.0 : 1.0; r[4] = c->qmax;
    r[5] = c->nBad; r[6] = c->iter; r[7] = c->done; r[8] = c->stop_out; r[9] = c->currentChi;
  }
  return t;
}
