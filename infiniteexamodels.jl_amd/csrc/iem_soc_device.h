// iem_soc_device.h — the kernels of the iem_soc object (include/iem.h): the second-order correction of the filter line search
// (Waechter and Biegler 2006, Algorithm A, steps A-5.5 to A-5.9; Ipopt's TrySecondOrderCorrection) beside iem_search — the gate
// (soc_open), the accumulated constraint residual and the corrected right-hand side (soc_rhs), the corrected trial point (soc_trial),
// the acceptance test of search_accept restated with the full step's alpha (soc_accept), and the copy of an accepted correction over
// the first-order direction (soc_select).  A code object of its own (no other source key knows of it), compiled with
// -ffp-contract=off; it has no sum and uses none of the helpers of iem_device.h: every line below is the order of operations of the
// contract in include/iem.h, each operation rounded once.
//
// NO ATOMIC, no inline assembly and no scratch in this file.  Every kernel is gated on the device by words 13–15 of the search
// object's control block (layout in include/iem.h) and returns BEFORE ITS FIRST STORE when it does not apply; the block is written
// with plain vector stores by one thread.
//
// soc_rhs / soc_trial / soc_select: the grid of the barrier object — one thread takes the entries i, i + stride, ... of
// [0, nvar + ncon): i < nvar is variable i, otherwise row j = i − nvar; fc bit 0 = lower bound of the row's slack present, bit 1 =
// upper, bit 2 = equality row.  Equality rows' entries of s, st, ds, dvL, dvU are neither read nor written.  soc_open, soc_accept:
// ONE workgroup of 64 threads.  soc_accept restates the test and the ballot / prefix-count filter compaction of search_accept
// (csrc/iem_search_device.h); tests/soc_reference.py calls the ONE numpy restatement of that test, which keeps the two in step.

#define SOC_SEARCHING 0ll
#define SOC_F_TYPE 1ll
#define SOC_H_TYPE 2ll
#define SOC_NONE 0ll
#define SOC_ACTIVE 1ll
#define SOC_ACCEPTED 2ll
#define SOC_CLOSED 3ll
#define SOC_ARMIJO_SLACK 0x1.4p-49      // 10·2⁻⁵²

// the control block: words of 8 bytes (those of csrc/iem_search_device.h, and the three of the correction)
enum { CW_ALPHA, CW_ALPHA_MAX, CW_PHI0, CW_THETA0, CW_SLOPE, CW_THETA_MIN, CW_THETA_MAX, CW_PHI_T, CW_THETA_T, CW_STATUS, CW_TRIALS, CW_COUNT, CW_FLAGS,
       CW_SOC_STATE, CW_SOC_ROUNDS, CW_SOC_ALPHA_PREV };

struct SocArgs {
  const double *rl, *ru, *ceq;                    // the barrier object's relaxed row bounds and the equality rows' right-hand side (ncon each)
  const unsigned char *fc;
  const double *x, *s, *y, *vL, *vU;              // the current point (rhs: s, y, vL, vU; trial: x, s)
  const double *c, *ct, *st_in, *rhs;             // rhs: c(x), c at the latest trial point, the slack there, the first-order right-hand side
  double *rhs_soc, *csoc;                         // rhs: nvar + ncon, and the object's accumulated residual (ncon)
  const double *sol, *ds, *dzL, *dzU, *dvL, *dvU; // the corrected direction (trial: sol, ds; select: all six)
  const double *alpha_soc;                        // {alpha_primal, alpha_dual} of barrier_step on the corrected direction
  double *xt, *st;                                // trial
  const double *ft, *merit;                       // accept: f at the trial point, {theta, sum log gap} there
  double *alpha_out;                              // accept: d_alpha (2)
  double *o_sol, *o_ds, *o_dzL, *o_dzU, *o_dvL, *o_dvU;      // select: the first-order direction
  double *ctl, *filter;                           // the search object's control block and filter
  double mu, sigma;
  double gamma_theta, gamma_phi, eta_phi, delta, s_theta, s_phi, kappa_soc;
  long long max_soc, capacity;
  long long nvar, n;
  const double *mu_blk;                           // iem_soc_bind_mu: the iem_mu block {mu, ...}, or null — then A.mu rules
};

__device__ __forceinline__ long long soc_word(const double *ctl, int w) { return __double_as_longlong(ctl[w]); }
__device__ __forceinline__ void soc_set_word(double *ctl, int w, long long v) { ctl[w] = __longlong_as_double(v); }
__device__ __forceinline__ double soc_abs(double a) { return __longlong_as_double(__double_as_longlong(a) & 0x7fffffffffffffffll); }
__device__ __forceinline__ bool soc_finite(double a) { return (__double_as_longlong(a) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll; }

// behind the first rung's accept: NONE becomes ACTIVE or CLOSED, any other state stays (a replayed graph finds it decided)
extern "C" __global__ __launch_bounds__(64) void soc_open(const SocArgs A) {
  double *ctl = A.ctl;
  if (threadIdx.x != 0 || soc_word(ctl, CW_SOC_STATE) != SOC_NONE) return;
  const double theta_t = ctl[CW_THETA_T], theta0 = ctl[CW_THETA0];
  const bool open = soc_word(ctl, CW_STATUS) == SOC_SEARCHING && soc_word(ctl, CW_TRIALS) == 1 && soc_finite(theta_t) && theta_t >= theta0;      // (a NaN compares false)
  if (open) {
    soc_set_word(ctl, CW_SOC_ROUNDS, 0);
    ctl[CW_SOC_ALPHA_PREV] = ctl[CW_ALPHA_MAX];
  }
  soc_set_word(ctl, CW_SOC_STATE, open ? SOC_ACTIVE : SOC_CLOSED);
}

extern "C" __global__ __launch_bounds__(256) void soc_rhs(const SocArgs A) {
  if (soc_word(A.ctl, CW_SOC_STATE) != SOC_ACTIVE) return;      // nothing is stored, csoc stays
  const bool first = soc_word(A.ctl, CW_SOC_ROUNDS) == 0;
  const double alpha_prev = A.ctl[CW_SOC_ALPHA_PREV], mu = A.mu_blk ? A.mu_blk[0] : A.mu;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      A.rhs_soc[i] = A.rhs[i];
      continue;
    }
    const long long j = i - A.nvar;
    const unsigned f = A.fc[j];
    if (f & 4) {
      const double ceq = A.ceq[j];
      const double prev = first ? A.c[j] - ceq : A.csoc[j];
      const double csoc = alpha_prev * prev + (A.ct[j] - ceq);
      A.csoc[j] = csoc;
      A.rhs_soc[i] = -csoc;
      continue;
    }
    const double s = A.s[j];
    const double prev = first ? A.c[j] - s : A.csoc[j];
    const double csoc = alpha_prev * prev + (A.ct[j] - A.st_in[j]);
    A.csoc[j] = csoc;
    double sl = 0.0, su = 0.0, ml = 0.0, mu_u = 0.0;
    if (f & 1) { const double e = s - A.rl[j]; sl = A.vL[j] / e; ml = mu / e; }
    if (f & 2) { const double e = A.ru[j] - s; su = A.vU[j] / e; mu_u = mu / e; }
    const double sigs = sl + su, gs = mu_u - ml;
    const double rs = gs - A.y[j], inv = 1.0 / sigs;
    A.rhs_soc[i] = -(csoc + rs * inv);
  }
}

extern "C" __global__ __launch_bounds__(256) void soc_trial(const SocArgs A) {
  if (soc_word(A.ctl, CW_SOC_STATE) != SOC_ACTIVE) return;
  const double alpha = A.alpha_soc[0];
  if (!(alpha > 0.0)) return;      // the barrier layer's "unusable": soc_accept closes the correction
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      A.xt[i] = A.x[i] + alpha * A.sol[i];
    } else {
      const long long j = i - A.nvar;
      if (A.fc[j] & 4) continue;
      A.st[j] = A.s[j] + alpha * A.ds[j];
    }
  }
}

extern "C" __global__ __launch_bounds__(64) void soc_accept(const SocArgs A) {
  double *ctl = A.ctl;
  const int lane = (int)threadIdx.x;
  if (soc_word(ctl, CW_SOC_STATE) != SOC_ACTIVE) return;      // nothing at all
  const long long rounds = soc_word(ctl, CW_SOC_ROUNDS);
  const double alpha_soc = A.alpha_soc[0], alpha_dual = A.alpha_soc[1];
  if (!(alpha_soc > 0.0)) {
    if (lane == 0) { soc_set_word(ctl, CW_SOC_ROUNDS, rounds + 1); soc_set_word(ctl, CW_SOC_STATE, SOC_CLOSED); }
    return;
  }
  // the test of search_accept, with the full step's alpha
  const double alpha = ctl[CW_ALPHA_MAX], phi0 = ctl[CW_PHI0], theta0 = ctl[CW_THETA0], slope = ctl[CW_SLOPE];
  const double theta_min = ctl[CW_THETA_MIN], theta_max = ctl[CW_THETA_MAX], theta_prev = ctl[CW_THETA_T];
  const long long flags = soc_word(ctl, CW_FLAGS);
  long long count = soc_word(ctl, CW_COUNT);
  count = count < 0 ? 0 : count > A.capacity ? A.capacity : count;
  const double theta_t = A.merit[0];
  const double phi_t = A.sigma * A.ft[0] - (A.mu_blk ? A.mu_blk[0] : A.mu) * A.merit[1];
  bool hit = false;
  for (long long k = lane; k < count; k += 64) hit = hit || (theta_t >= A.filter[2 * k] && phi_t >= A.filter[2 * k + 1]);
  const bool dominated = __ballot(hit) != 0ull;
  const bool admissible = soc_finite(phi_t) && soc_finite(theta_t) && theta_t <= theta_max && !dominated;
  const bool switching = slope < 0.0 && theta0 <= theta_min && alpha * pow(-slope, A.s_phi) > A.delta * pow(theta0, A.s_theta);
  const bool armijo = phi_t <= (phi0 + (A.eta_phi * alpha) * slope) + SOC_ARMIJO_SLACK * soc_abs(phi0);
  const double f_theta = (1.0 - A.gamma_theta) * theta0, f_phi = phi0 - A.gamma_phi * theta0;
  const bool sufficient = theta_t <= f_theta || phi_t <= f_phi;
  const bool f_type = admissible && switching && armijo;
  const bool h_type = admissible && !switching && sufficient;
  if (lane == 0) { ctl[CW_PHI_T] = phi_t; ctl[CW_THETA_T] = theta_t; soc_set_word(ctl, CW_SOC_ROUNDS, rounds + 1); }
  if (!f_type && !h_type) {      // rejected: another round, or the correction closes and backtracking goes on from the block's alpha
    if (lane == 0) {
      const bool go_on = rounds + 1 < A.max_soc && soc_finite(theta_t) && theta_t <= A.kappa_soc * theta_prev;
      if (go_on) ctl[CW_SOC_ALPHA_PREV] = alpha_soc;
      else soc_set_word(ctl, CW_SOC_STATE, SOC_CLOSED);
    }
    return;
  }
  if (h_type) {      // the filter gains (f_theta, f_phi), exactly as in search_accept
    long long kept = 0;
    for (long long base = 0; base < count; base += 64) {
      const long long k = base + lane;
      double e_theta = 0.0, e_phi = 0.0;
      bool keep = false;
      if (k < count) {
        e_theta = A.filter[2 * k];
        e_phi = A.filter[2 * k + 1];
        keep = !(e_theta >= f_theta && e_phi >= f_phi);
      }
      const unsigned long long m = __ballot(keep);
      if (keep) {
        const long long at = kept + __popcll(m & ((1ull << lane) - 1ull));
        A.filter[2 * at] = e_theta;
        A.filter[2 * at + 1] = e_phi;
      }
      kept += __popcll(m);
    }
    if (lane == 0) {
      if (kept < A.capacity) {
        A.filter[2 * kept] = f_theta;
        A.filter[2 * kept + 1] = f_phi;
        soc_set_word(ctl, CW_COUNT, kept + 1);
      } else {      // a full filter: the step still stands
        soc_set_word(ctl, CW_COUNT, kept);
        soc_set_word(ctl, CW_FLAGS, flags | 2);
      }
    }
  }
  if (lane == 0) {
    soc_set_word(ctl, CW_STATUS, f_type ? SOC_F_TYPE : SOC_H_TYPE);
    ctl[CW_ALPHA] = alpha_soc;
    A.alpha_out[0] = alpha_soc;
    A.alpha_out[1] = alpha_dual;
    soc_set_word(ctl, CW_SOC_STATE, SOC_ACCEPTED);
  }
}

extern "C" __global__ __launch_bounds__(256) void soc_select(const SocArgs A) {
  if (soc_word(A.ctl, CW_SOC_STATE) != SOC_ACCEPTED) return;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    A.o_sol[i] = A.sol[i];
    if (i < A.nvar) {
      A.o_dzL[i] = A.dzL[i];
      A.o_dzU[i] = A.dzU[i];
    } else {
      const long long j = i - A.nvar;
      if (A.fc[j] & 4) continue;
      A.o_ds[j] = A.ds[j];
      A.o_dvL[j] = A.dvL[j];
      A.o_dvU[j] = A.dvU[j];
    }
  }
}
