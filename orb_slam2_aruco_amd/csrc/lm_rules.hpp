// lm_rules.hpp -- g2o's OptimizationAlgorithmLevenberg as the three optimizers on the device run it (pose_optimizer.hip,
// sim3_optimizer.hip, local_ba.hip): the scalar state of one optimize() and the five steps that change it.  What is damped, solved
// and summed differs between them (a dense 6 x 6 or 7 x 7 system in one workgroup, a Schur complement over a chain of kernels); these
// rules do not.  Plain scalar arithmetic, no HIP: lba_plan.hpp embeds the state in LbaCtl, and tests/lba_plan_driver.cpp compiles
// that header with g++.  The CPU restatements of tests/ state the same rules in their own words (tests/g2o_ref.hpp) and share nothing
// with this file.
#pragma once
#include <cfloat>
#include <cmath>

#include "../../include/orbfe_math.h"   // ORBFE_HD

namespace orbfe {

struct LmState {
    double lambda, ni, currentChi, iniChi, rho;
    int q, nbad_lm;   // trials of this iteration; iterations in a row that gained less than a thousandth
};
static_assert(sizeof(LmState) == 48, "the control blocks that embed it keep their sizes");

// optimize() begins
ORBFE_HD void lm_round_start(LmState& c)
{
    c.lambda = 0;
    c.ni = 2;
    c.nbad_lm = 0;
    c.rho = 0;
}

// after a linearisation with robust chi2 `chi`; `first`: the round's first iteration, maxdiag = max |H_jj| (read only then)
ORBFE_HD void lm_linearised(LmState& c, double chi, bool first, double maxdiag)
{
    c.currentChi = c.iniChi = chi;
    if (first) {
        c.lambda = 1e-5 * maxdiag;
        c.ni = 2;
        c.nbad_lm = 0;
    }
    c.rho = 0;
    c.q = 0;
}

// the same behind setUserLambdaInit(user_lambda): computeLambdaInit returns the user's value instead of 1e-5 max |H_jj|
// (essential_graph.hip: 1e-16)
ORBFE_HD void lm_linearised_user(LmState& c, double chi, bool first, double user_lambda)
{
    lm_linearised(c, chi, false, 0.);
    if (first) {
        c.lambda = user_lambda;
        c.ni = 2;
        c.nbad_lm = 0;
    }
}

// A trial with robust chi2 tempChi; solved: the damped system was positive; scale = sum x (lambda x + b) over every update, to
// which g2o's 1e-3 is added here, last.  Returns whether the trial is accepted; the caller restores its estimate when it is not.
ORBFE_HD bool lm_judge_trial(LmState& c, double tempChi, bool solved, double scale)
{
    if (!solved) tempChi = DBL_MAX;
    double rho = c.currentChi - tempChi;
    scale += 1e-3;
    rho /= scale;
    const bool accepted = rho > 0 && std::isfinite(tempChi);
    if (accepted) {
        double alpha = 1. - std::pow((2 * rho - 1), 3.0);
        alpha = std::fmin(alpha, 2. / 3.);
        const double sf = std::fmax(1. / 3., alpha);
        c.lambda *= sf;
        c.ni = 2;
        c.currentChi = tempChi;
    } else {
        c.lambda *= c.ni;
        c.ni *= 2;
    }
    c.rho = rho;
    c.q++;
    return accepted;
}

// another trial in this iteration?
ORBFE_HD bool lm_try_again(const LmState& c) { return c.rho < 0 && c.q < 10; }

// the iteration is over: whether optimize() stops here
ORBFE_HD bool lm_iteration_end(LmState& c)
{
    bool stop = c.q == 10 || c.rho == 0;
    if (!stop) {
        if ((c.iniChi - c.currentChi) * 1e3 < c.iniChi) c.nbad_lm++;
        else c.nbad_lm = 0;
        stop = c.nbad_lm >= 3;
    }
    return stop;
}

} // namespace orbfe
