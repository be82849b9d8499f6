// iem_search_device.h — the kernels of the iem_search object (include/iem.h): the filter line search of a primal-dual interior-point
// iteration on the device — the slope of the barrier objective along the direction and the set-up of a search (search_begin), the
// trial point (search_trial), and the acceptance test of Waechter and Biegler 2006, Algorithm A, with its filter (search_accept).
// A code object of its own (no other source key knows of it), compiled with -ffp-contract=off behind the helpers of iem_device.h
// (everything in front of its own kernels, with IEM_TILE = 256): every line below is the order of operations of the contract in
// include/iem.h, each operation rounded once.
//
// NO FLOAT ATOMIC, no inline assembly and no scratch in this file.  The one sum (the slope) goes through iem_shared_park /
// iem_shared_last / iem_shared_totals of iem_device.h as they stand: a lane adds its entries in index order, the workgroup parks its
// total, the workgroup that arrives last totals the column in a fixed order — bitwise reproducible, one launch; the partials and the
// tickets belong to the object and reset themselves.  Every decision is taken on the device from the control block (16 words of 8
// bytes, layout in include/iem.h) and written back to it with plain vector stores by one thread.
//
// search_begin / search_trial: the grid of the barrier object — one thread takes the entries i, i + stride, ... of [0, nvar + ncon):
// i < nvar is variable i, otherwise row j = i − nvar; flags as there (fx / fc bit 0 = lower bound present, bit 1 = upper, fc bit 2 =
// equality row).  Equality rows' entries of s, ds, st are neither read nor written.  search_accept: ONE workgroup of 64 threads.

#define SEARCH_SEARCHING 0ll
#define SEARCH_F_TYPE 1ll
#define SEARCH_H_TYPE 2ll
#define SEARCH_FAILED 3ll
#define SEARCH_UNUSABLE 4ll
#define SEARCH_NAN_BITS 0x7ff8000000000000ll
#define SEARCH_ARMIJO_SLACK 0x1.4p-49      // 10·2⁻⁵²

// the control block: words of 8 bytes
enum { SW_ALPHA, SW_ALPHA_MAX, SW_PHI0, SW_THETA0, SW_SLOPE, SW_THETA_MIN, SW_THETA_MAX, SW_PHI_T, SW_THETA_T, SW_STATUS, SW_TRIALS, SW_COUNT, SW_FLAGS };

struct SearchArgs {
  const double *xl, *xu, *rl, *ru;                // the barrier object's relaxed bounds (nvar, nvar, ncon, ncon)
  const unsigned char *fx, *fc;
  const double *x, *s, *g, *sol, *ds;             // the point, grad f (begin), [dx; dy], ds
  const double *obj, *err, *alpha_in;             // begin: f, the eight numbers of barrier_error, {alpha_primal, alpha_dual}
  double *xt, *st;                                // trial
  const double *ft, *merit;                       // accept: f at the trial point, {theta, sum log gap} there
  double *alpha_out;                              // accept: d_alpha[0]
  double *ctl, *filter;                           // the control block, `capacity` pairs (theta, phi)
  double *red;                                    // n_wg parked values, then the ticket words
  const long long *tab;                           // offs | first | count of iem_shared_totals: {0, 0, n_wg}
  double mu, sigma;
  double gamma_theta, gamma_phi, eta_phi, delta, s_theta, s_phi, alpha_floor;
  long long max_trials, capacity;
  long long nvar, n, n_wg;
  const double *mu_blk;                           // iem_search_bind_mu: the iem_mu block {mu, ...}, or null — then A.mu rules
};

__device__ __forceinline__ long long search_word(const double *ctl, int w) { return __double_as_longlong(ctl[w]); }
__device__ __forceinline__ void search_set_word(double *ctl, int w, long long v) { ctl[w] = __longlong_as_double(v); }
__device__ __forceinline__ double search_abs(double a) { return __longlong_as_double(__double_as_longlong(a) & 0x7fffffffffffffffll); }
__device__ __forceinline__ bool search_finite(double a) { return (__double_as_longlong(a) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll; }

extern "C" __global__ __launch_bounds__(256) void search_begin(const SearchArgs A) {
  __shared__ double lds[8];
  const long long stride = (long long)gridDim.x * 256;
  const double mu = A.mu_blk ? A.mu_blk[0] : A.mu, sigma = A.sigma;
  double v[1] = {0.0};      // the slope: the terms of this lane in index order
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const bool hl = A.fx[i] & 1, hu = A.fx[i] & 2;
      const double x = A.x[i];
      double ml = 0.0, mu_u = 0.0;
      if (hl) { const double d = x - A.xl[i]; ml = mu / d; }
      if (hu) { const double d = A.xu[i] - x; mu_u = mu / d; }
      const double gb = mu_u - ml;
      v[0] += (sigma * A.g[i] + gb) * A.sol[i];
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      if (f & 4) continue;
      const double s = A.s[j];
      double ml = 0.0, mu_u = 0.0;
      if (f & 1) { const double e = s - A.rl[j]; ml = mu / e; }
      if (f & 2) { const double e = A.ru[j] - s; mu_u = mu / e; }
      const double gs = mu_u - ml;
      v[0] += gs * A.ds[j];
    }
  }
  iem_shared_park<1>(v, A.red, A.tab, (long long)blockIdx.x, lds);
  if (!iem_shared_last(A.red + A.n_wg, (long long)blockIdx.x, A.n_wg, lds + 7)) return;
  iem_shared_totals(1, A.red, A.tab, A.tab + 1, A.tab + 2, lds);
  if (threadIdx.x != 0) return;
  // the control block of this search; the filter, its count and the flags stay
  double *ctl = A.ctl;
  const double slope = lds[0], amax = A.alpha_in[0], theta0 = A.err[6];
  const bool usable = amax > 0.0 && slope == slope;      // a step length of +0.0 (or a NaN): the state or the direction was unusable
  ctl[SW_ALPHA] = usable ? amax : 0.0;
  ctl[SW_ALPHA_MAX] = amax;
  ctl[SW_PHI0] = sigma * A.obj[0] - mu * A.err[7];
  ctl[SW_THETA0] = theta0;
  ctl[SW_SLOPE] = slope;
  const long long flags = search_word(ctl, SW_FLAGS);
  if (!(flags & 1)) {
    const double t1 = theta0 > 1.0 ? theta0 : 1.0;
    ctl[SW_THETA_MIN] = 1e-4 * t1;
    ctl[SW_THETA_MAX] = 1e4 * t1;
    search_set_word(ctl, SW_FLAGS, flags | 1);
  }
  search_set_word(ctl, SW_PHI_T, SEARCH_NAN_BITS);      // no trial yet
  search_set_word(ctl, SW_THETA_T, SEARCH_NAN_BITS);
  search_set_word(ctl, SW_STATUS, usable ? SEARCH_SEARCHING : SEARCH_UNUSABLE);
  search_set_word(ctl, SW_TRIALS, 0);
  ctl[13] = 0.0; ctl[14] = 0.0; ctl[15] = 0.0;
}

extern "C" __global__ __launch_bounds__(256) void search_trial(const SearchArgs A) {
  const long long status = search_word(A.ctl, SW_STATUS);
  if (status == SEARCH_FAILED || status == SEARCH_UNUSABLE) return;      // nothing is stored
  const double alpha = A.ctl[SW_ALPHA];
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

extern "C" __global__ __launch_bounds__(64) void search_accept(const SearchArgs A) {
  double *ctl = A.ctl;
  const int lane = (int)threadIdx.x;
  const long long status = search_word(ctl, SW_STATUS);
  if (status != SEARCH_SEARCHING) {      // decided already: the same bits every time, nothing else
    if (lane == 0) A.alpha_out[0] = (status == SEARCH_F_TYPE || status == SEARCH_H_TYPE) ? ctl[SW_ALPHA] : 0.0;
    return;
  }
  const double alpha = ctl[SW_ALPHA], phi0 = ctl[SW_PHI0], theta0 = ctl[SW_THETA0], slope = ctl[SW_SLOPE];
  const double theta_min = ctl[SW_THETA_MIN], theta_max = ctl[SW_THETA_MAX];
  const long long trials = search_word(ctl, SW_TRIALS), flags = search_word(ctl, SW_FLAGS);
  long long count = search_word(ctl, SW_COUNT);      // (a host may write the block: a count outside the filter reads and writes nothing outside it)
  count = count < 0 ? 0 : count > A.capacity ? A.capacity : count;
  const double theta_t = A.merit[0];
  const double phi_t = A.sigma * A.ft[0] - (A.mu_blk ? A.mu_blk[0] : A.mu) * A.merit[1];
  // admissible: finite, theta below its ceiling, not dominated by a filter entry (the scan: lane l takes the entries l, l + 64, ...)
  bool hit = false;
  for (long long k = lane; k < count; k += 64) hit = hit || (theta_t >= A.filter[2 * k] && phi_t >= A.filter[2 * k + 1]);
  const bool dominated = __ballot(hit) != 0ull;
  const bool admissible = search_finite(phi_t) && search_finite(theta_t) && theta_t <= theta_max && !dominated;
  const bool switching = slope < 0.0 && theta0 <= theta_min && alpha * pow(-slope, A.s_phi) > A.delta * pow(theta0, A.s_theta);
  const bool armijo = phi_t <= (phi0 + (A.eta_phi * alpha) * slope) + SEARCH_ARMIJO_SLACK * search_abs(phi0);
  const double f_theta = (1.0 - A.gamma_theta) * theta0, f_phi = phi0 - A.gamma_phi * theta0;
  const bool sufficient = theta_t <= f_theta || phi_t <= f_phi;
  const bool f_type = admissible && switching && armijo;
  const bool h_type = admissible && !switching && sufficient;
  if (lane == 0) { ctl[SW_PHI_T] = phi_t; ctl[SW_THETA_T] = theta_t; }
  if (f_type) {
    if (lane == 0) { search_set_word(ctl, SW_STATUS, SEARCH_F_TYPE); A.alpha_out[0] = alpha; }
    return;
  }
  if (!h_type) {      // rejected: the next rung tries half the step; d_alpha[0] stays safe for an update in between
    if (lane == 0) {
      const double half = 0.5 * alpha;
      const bool failed = trials + 1 == A.max_trials || half < A.alpha_floor;
      search_set_word(ctl, SW_TRIALS, trials + 1);
      ctl[SW_ALPHA] = failed ? 0.0 : half;
      if (failed) search_set_word(ctl, SW_STATUS, SEARCH_FAILED);
      A.alpha_out[0] = 0.0;
    }
    return;
  }
  // h-type: the filter gains (f_theta, f_phi) — the entries it dominates leave first, the others keep their order (64 entries per
  // pass: every lane has loaded its entry before any lane stores one, and a store never lands behind the pass it belongs to)
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
      search_set_word(ctl, SW_COUNT, kept + 1);
    } else {      // a full filter: the step still stands
      search_set_word(ctl, SW_COUNT, kept);
      search_set_word(ctl, SW_FLAGS, flags | 2);
    }
    search_set_word(ctl, SW_STATUS, SEARCH_H_TYPE);
    A.alpha_out[0] = alpha;
  }
}
