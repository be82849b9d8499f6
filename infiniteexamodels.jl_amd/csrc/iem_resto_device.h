// iem_resto_device.h — the kernels of the iem_resto object (include/iem.h): the feasibility restoration phase of a primal-dual
// interior-point method (Waechter and Biegler 2006, step A-9; Ipopt's section 3.3) on the device.  With the elastic variables p, n of
// the restoration problem  min rho sum(p + n) + zeta/2 |D_R (x - x_R)|^2  s.t.  c(x) - s - p + n = 0,  p, n >= 0  eliminated, its
// Newton system is the one iem_kkt_assemble_diag / iem_kkt_solve_refined_diag solve; this file is the element-wise layer around it:
// the elastic start (resto_enter), the diagonal and the right-hand side (resto_terms), the directions and the step lengths
// (resto_step), the restoration's merit sums (resto_merit), its slope and the set-up of the inner search (resto_begin), the trial
// point (resto_trial), the update (resto_update), the error terms (resto_error), the return test against the ORIGINAL filter
// (resto_check), and the multiplier reset on the way out (resto_leave_max, resto_leave).  A code object of its own (no other source
// key knows of it), compiled with -ffp-contract=off behind the helpers of iem_device.h (everything in front of its own kernels, with
// IEM_TILE = 256): every line below is the order of operations of the contract in include/iem.h, each operation rounded once.
//
// NO FLOAT ATOMIC, no inline assembly and no scratch in this file: the only atomics are integer atomicMin (resto_step) and atomicMax
// (resto_error, resto_leave_max) on the bit pattern of a non-negative double, at most ONE per workgroup and slot (the scheme of
// bar_extremes in iem_barrier_device.h: shuffles, LDS, a relaxed look at the slot).  The sums go through iem_shared_park /
// iem_shared_last / iem_shared_totals of iem_device.h as they stand: a lane adds its entries in index order, every workgroup parks
// its values, the workgroup that arrives last totals each column in a fixed order — bitwise reproducible, one launch.
//
// One thread takes the entries i, i + stride, ... of [0, nvar + ncon): i < nvar is variable i, otherwise row j = i − nvar.  Plain
// vector loads and stores.  Flags as in the barrier kernels: fx[i] bit 0 = lower bound present, bit 1 = upper; fc[j] the same for an
// inequality row's slack, bit 2 = equality row.  Entries of the slack-side vectors (s, vL, vU, ds, dvL, dvU, st, sR, ws) on equality
// rows are neither read nor written, a multiplier is read only where its bound is present, and an absent bound contributes an exact
// +0.0.  resto_enter_filter and resto_check: ONE workgroup of 64 threads.

#define RES_ONE_BITS 0x3ff0000000000000ull   // 1.0
#define RES_NAN_BITS 0x7ff8000000000000ll
#define RES_NONE 0ll
#define RES_ACTIVE 1ll
#define RES_RETURN 2ll
#define RES_SEARCHING 0ll
#define RES_FAILED 3ll
#define RES_UNUSABLE 4ll

// the object's block (words of 8 bytes) and the words of a search's control block this file reads or writes
enum { RW_STATE, RW_THETA_START, RW_THETA, RW_PHI, RW_ZMAX };
enum { SW_ALPHA, SW_ALPHA_MAX, SW_PHI0, SW_THETA0, SW_SLOPE, SW_THETA_MIN, SW_THETA_MAX, SW_PHI_T, SW_THETA_T, SW_STATUS, SW_TRIALS, SW_COUNT, SW_FLAGS };

struct RestoArgs {
  const double *xl, *xu, *rl, *ru, *ceq;          // the barrier object's relaxed bounds and the equality rows' right-hand side
  const unsigned char *fx, *fc;
  double *x, *s, *y, *zL, *zU, *vL, *vU;          // the state (enter / update / leave write it, the others read it)
  const double *r, *c, *sol;                      // J'y (nvar, may be null in resto_error), c(x) (ncon), [dx; dy]
  double *ds, *dzL, *dzU, *dvL, *dvU;             // the directions (resto_step writes, resto_update reads)
  double *sigma, *dcon, *rhs;                     // resto_terms
  unsigned long long *alpha;                      // {alpha_primal, alpha_dual} as bit patterns
  double *out;                                    // resto_error: 8, resto_merit: 3
  double *xt, *st;                                // resto_trial
  const double *merit0, *f, *merit;               // resto_begin: the three numbers of resto_merit(0); resto_check: f, {theta, sum log gap}
  double *p, *n_, *zp, *zn, *dp, *dn, *dzp, *dzn, *pt, *nt, *sR, *ws, *xR, *wx;      // the object's vectors
  double *blk;                                    // the object's block
  double *octl, *ofilter;                         // the ORIGINAL search: control block, filter
  double *ictl;                                   // the INNER search: control block
  double *red;                                    // 4 n_wg parked values, then the ticket words (the object's own)
  const long long *tab;                           // offs[4] | first[4] | count[4] of iem_shared_totals (the barrier object's)
  double mu, tau, kappa, zeta, rho, kappa_resto, threshold, gamma_theta, gamma_phi;
  long long capacity, which;
  long long nvar, n, n_wg;
};

// np.maximum / np.minimum: a NaN in either operand gives a NaN
__device__ __forceinline__ double res_max(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double res_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double res_abs(double a) { return __longlong_as_double(__double_as_longlong(a) & 0x7fffffffffffffffll); }
__device__ __forceinline__ unsigned long long res_abs_bits(double a) { return (unsigned long long)__double_as_longlong(a) & 0x7fffffffffffffffull; }
__device__ __forceinline__ bool res_finite(double a) { return (__double_as_longlong(a) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll; }
// a step-length candidate: its bit pattern, or 0 when it is not > 0 (a NaN, a point on or outside its bound)
__device__ __forceinline__ unsigned long long res_cand(double a) { return a > 0.0 ? (unsigned long long)__double_as_longlong(a) : 0ull; }
__device__ __forceinline__ unsigned long long res_umin(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned long long res_umax(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ long long res_word(const double *ctl, int w) { return __double_as_longlong(ctl[w]); }
__device__ __forceinline__ void res_set_word(double *ctl, int w, long long v) { ctl[w] = __longlong_as_double(v); }

// The extremes of the workgroup into their slots: per wave by shuffles, across the waves through LDS (NV·4 words), then thread s < NV
// holds value s of the workgroup and issues ONE integer atomic — and none where a relaxed agent-scope look at the slot shows that it
// would not change it (the slot only ever moves towards the extreme, so a stale look can only cost an atomic, never lose a value).
template <int NV, bool IS_MIN>
__device__ __forceinline__ void res_extremes(unsigned long long (&v)[NV], unsigned long long *slots, unsigned long long *lds) {
  constexpr int NW = IEM_TILE / IEM_WAVE;
#pragma unroll
  for (int s = 0; s < NV; ++s) {
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(v[s], o, 64);
      v[s] = IS_MIN ? res_umin(v[s], other) : res_umax(v[s], other);
    }
    if (iem_lane() == 0) lds[iem_wave() * NV + s] = v[s];
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int s = (int)threadIdx.x;
    unsigned long long b = lds[s];
    for (int w = 1; w < NW; ++w) b = IS_MIN ? res_umin(b, lds[w * NV + s]) : res_umax(b, lds[w * NV + s]);
    const unsigned long long cur = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (IS_MIN) { if (b < cur) atomicMin(slots + s, b); }
    else if (b > cur) atomicMax(slots + s, b);
  }
}

// the sums of the launch: parked per workgroup, totalled by the workgroup that arrives last (lds: 4 (NW + 1) + 1 doubles)
template <int NV>
__device__ __forceinline__ bool res_sums(const RestoArgs &A, const double (&v)[NV], double *lds) {
  iem_shared_park<NV>(v, A.red, A.tab, (long long)blockIdx.x, lds);
  if (!iem_shared_last(A.red + 4 * A.n_wg, (long long)blockIdx.x, A.n_wg, lds + 20)) return false;
  iem_shared_totals(NV, A.red, A.tab, A.tab + 4, A.tab + 8, lds);
  return true;
}

// the safeguard of Ipopt's eq. (16):  z = min(max(z, mu / (kappa gap)), (kappa mu) / gap)
__device__ __forceinline__ double res_guard(double z, double gap, double mu, double kappa) {
  return res_min(res_max(z, mu / (kappa * gap)), (kappa * mu) / gap);
}

// the proximity weight  m·m  with  m = min(1, 1/|v|)
__device__ __forceinline__ double res_weight(double v) {
  const double m = res_min(1.0, 1.0 / res_abs(v));
  return m * m;
}

// what every row needs of the elastic side
struct ResRow { double p, n, zp, zn, rc, Dp, Dn, ep, en; };
__device__ __forceinline__ ResRow res_row(const RestoArgs &A, long long j, double inf, double y, double mu) {
  ResRow q;
  q.p = A.p[j]; q.n = A.n_[j]; q.zp = A.zp[j]; q.zn = A.zn[j];
  q.rc = (inf - q.p) + q.n;
  q.Dp = q.p / q.zp;
  q.Dn = q.n / q.zn;
  q.ep = (mu - q.p * (A.rho - y)) / q.zp;
  q.en = (mu - q.n * (A.rho + y)) / q.zn;
  return q;
}

extern "C" __global__ __launch_bounds__(256) void resto_enter(const RestoArgs A) {
  const long long stride = (long long)gridDim.x * 256;
  const double mu = A.mu, rho = A.rho, rho2 = 2.0 * A.rho;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const unsigned f = A.fx[i];
      const double x = A.x[i];
      A.xR[i] = x;
      A.wx[i] = res_weight(x);
      if (f & 1) A.zL[i] = res_min(rho, A.zL[i]);
      if (f & 2) A.zU[i] = res_min(rho, A.zU[i]);
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      double inf;
      if (f & 4) {
        inf = A.c[j] - A.ceq[j];
      } else {
        const double s = A.s[j];
        inf = A.c[j] - s;
        A.sR[j] = s;
        A.ws[j] = res_weight(s);
        if (f & 1) A.vL[j] = res_min(rho, A.vL[j]);
        if (f & 2) A.vU[j] = res_min(rho, A.vU[j]);
      }
      const double h = (mu - rho * inf) / rho2;
      const double n = h + sqrt(h * h + (mu * inf) / rho2);
      const double p = inf + n;
      A.n_[j] = n;
      A.p[j] = p;
      A.zp[j] = mu / p;
      A.zn[j] = mu / n;
      A.y[j] = 0.0;
    }
  }
}

// the ORIGINAL filter gains ((1 − gamma_theta)·theta0, phi0 − gamma_phi·theta0) of the ORIGINAL block — the rule of search_accept's
// h-type branch: the entries it dominates leave first, the others keep their order, a full filter sets flag bit 1
extern "C" __global__ __launch_bounds__(64) void resto_enter_filter(const RestoArgs A) {
  double *ctl = A.octl;
  const int lane = (int)threadIdx.x;
  const double theta0 = ctl[SW_THETA0], phi0 = ctl[SW_PHI0];
  const long long flags = res_word(ctl, SW_FLAGS);
  long long count = res_word(ctl, SW_COUNT);
  count = count < 0 ? 0 : count > A.capacity ? A.capacity : count;
  const double f_theta = (1.0 - A.gamma_theta) * theta0, f_phi = phi0 - A.gamma_phi * theta0;
  long long kept = 0;
  for (long long base = 0; base < count; base += 64) {
    const long long k = base + lane;
    double e_theta = 0.0, e_phi = 0.0;
    bool keep = false;
    if (k < count) {
      e_theta = A.ofilter[2 * k];
      e_phi = A.ofilter[2 * k + 1];
      keep = !(e_theta >= f_theta && e_phi >= f_phi);
    }
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const long long at = kept + __popcll(m & ((1ull << lane) - 1ull));
      A.ofilter[2 * at] = e_theta;
      A.ofilter[2 * at + 1] = e_phi;
    }
    kept += __popcll(m);
  }
  if (lane == 0) {
    if (kept < A.capacity) {
      A.ofilter[2 * kept] = f_theta;
      A.ofilter[2 * kept + 1] = f_phi;
      res_set_word(ctl, SW_COUNT, kept + 1);
    } else {
      res_set_word(ctl, SW_COUNT, kept);
      res_set_word(ctl, SW_FLAGS, flags | 2);
    }
    A.blk[RW_THETA_START] = theta0;
    res_set_word(A.blk, RW_THETA, RES_NAN_BITS);      // no check yet
    res_set_word(A.blk, RW_PHI, RES_NAN_BITS);
    res_set_word(A.blk, RW_STATE, RES_ACTIVE);
  }
}

extern "C" __global__ __launch_bounds__(256) void resto_terms(const RestoArgs A) {
  const long long stride = (long long)gridDim.x * 256;
  const double mu = A.mu, zeta = A.zeta;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const bool hl = A.fx[i] & 1, hu = A.fx[i] & 2;
      const double x = A.x[i];
      double sl = 0.0, su = 0.0, ml = 0.0, mu_u = 0.0;
      if (hl) { const double d = x - A.xl[i]; sl = A.zL[i] / d; ml = mu / d; }
      if (hu) { const double d = A.xu[i] - x; su = A.zU[i] / d; mu_u = mu / d; }
      const double zw = zeta * A.wx[i];
      A.sigma[i] = (sl + su) + zw;
      const double gx = (mu_u - ml) + zw * (x - A.xR[i]);
      A.rhs[i] = -(A.r[i] + gx);
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      const double y = A.y[j];
      if (f & 4) {
        const ResRow q = res_row(A, j, A.c[j] - A.ceq[j], y, mu);
        const double t = (q.rc - q.ep) + q.en;
        A.dcon[j] = q.Dp + q.Dn;
        A.rhs[i] = -t;
        continue;
      }
      const double s = A.s[j];
      const ResRow q = res_row(A, j, A.c[j] - s, y, mu);
      const double t = (q.rc - q.ep) + q.en, D = q.Dp + q.Dn;
      double sl = 0.0, su = 0.0, ml = 0.0, mu_u = 0.0;
      if (f & 1) { const double e = s - A.rl[j]; sl = A.vL[j] / e; ml = mu / e; }
      if (f & 2) { const double e = A.ru[j] - s; su = A.vU[j] / e; mu_u = mu / e; }
      const double sigs = sl + su, gs = mu_u - ml;
      const double zs = zeta * A.ws[j];
      const double sigs1 = sigs + zs;
      const double gsr = gs + zs * (s - A.sR[j]);
      const double rs1 = gsr - y, inv = 1.0 / sigs1;
      A.dcon[j] = inv + D;
      A.rhs[i] = -(t + rs1 * inv);
    }
  }
}

extern "C" __global__ __launch_bounds__(256) void resto_step(const RestoArgs A) {
  __shared__ unsigned long long lds[2 * (IEM_TILE / IEM_WAVE)];
  const long long stride = (long long)gridDim.x * 256;
  const double mu = A.mu, tau = A.tau, ntau = -A.tau, zeta = A.zeta;
  unsigned long long ap = RES_ONE_BITS, ad = RES_ONE_BITS;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const bool hl = A.fx[i] & 1, hu = A.fx[i] & 2;
      const double x = A.x[i], dx = A.sol[i];
      double dzl = 0.0, dzu = 0.0;
      if (dx != dx) ap = 0ull;      // a NaN in the direction: unusable, whatever the bounds
      if (hl) {
        const double d = x - A.xl[i], z = A.zL[i];
        dzl = (mu / d - z) - (z / d) * dx;
        if (dx < 0.0) ap = res_umin(ap, res_cand((ntau * d) / dx));
        if (dzl < 0.0) ad = res_umin(ad, res_cand((ntau * z) / dzl));
        if (dzl != dzl) ad = 0ull;
      }
      if (hu) {
        const double d = A.xu[i] - x, z = A.zU[i];
        dzu = (mu / d - z) + (z / d) * dx;
        if (dx > 0.0) ap = res_umin(ap, res_cand((tau * d) / dx));
        if (dzu < 0.0) ad = res_umin(ad, res_cand((ntau * z) / dzu));
        if (dzu != dzu) ad = 0ull;
      }
      A.dzL[i] = dzl;
      A.dzU[i] = dzu;
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      const double dy = A.sol[i], y = A.y[j];
      if (dy != dy) ap = 0ull;
      // the elastic side: every row has it
      const ResRow q = res_row(A, j, 0.0, y, mu);      // (rc is not needed here: c is not read)
      const double dp = q.ep + q.Dp * dy;
      const double dn = q.en - q.Dn * dy;
      const double dzp = ((A.rho - y) - q.zp) - dy;
      const double dzn = ((A.rho + y) - q.zn) + dy;
      A.dp[j] = dp; A.dn[j] = dn; A.dzp[j] = dzp; A.dzn[j] = dzn;
      if (dp < 0.0) ap = res_umin(ap, res_cand((ntau * q.p) / dp));
      if (dn < 0.0) ap = res_umin(ap, res_cand((ntau * q.n) / dn));
      if (dp != dp || dn != dn) ap = 0ull;
      if (dzp < 0.0) ad = res_umin(ad, res_cand((ntau * q.zp) / dzp));
      if (dzn < 0.0) ad = res_umin(ad, res_cand((ntau * q.zn) / dzn));
      if (dzp != dzp || dzn != dzn) ad = 0ull;
      if (f & 4) continue;
      const bool gl = f & 1, gu = f & 2;
      const double s = A.s[j];
      double el = 0.0, eu = 0.0, vl = 0.0, vu = 0.0, sl = 0.0, su = 0.0, ml = 0.0, mu_u = 0.0;
      if (gl) { el = s - A.rl[j]; vl = A.vL[j]; sl = vl / el; ml = mu / el; }
      if (gu) { eu = A.ru[j] - s; vu = A.vU[j]; su = vu / eu; mu_u = mu / eu; }
      const double sigs = sl + su, gs = mu_u - ml;
      const double zs = zeta * A.ws[j];
      const double sigs1 = sigs + zs;
      const double gsr = gs + zs * (s - A.sR[j]);
      const double rs1 = gsr - y;
      const double ds = (dy - rs1) / sigs1;
      A.ds[j] = ds;
      if (ds != ds) ap = 0ull;
      double dvl = 0.0, dvu = 0.0;
      if (gl) {
        dvl = (ml - vl) - sl * ds;
        if (ds < 0.0) ap = res_umin(ap, res_cand((ntau * el) / ds));
        if (dvl < 0.0) ad = res_umin(ad, res_cand((ntau * vl) / dvl));
        if (dvl != dvl) ad = 0ull;
      }
      if (gu) {
        dvu = (mu_u - vu) + su * ds;
        if (ds > 0.0) ap = res_umin(ap, res_cand((tau * eu) / ds));
        if (dvu < 0.0) ad = res_umin(ad, res_cand((ntau * vu) / dvu));
        if (dvu != dvu) ad = 0ull;
      }
      A.dvL[j] = dvl;
      A.dvU[j] = dvu;
    }
  }
  unsigned long long a[2] = {ap, ad};      // the slots were seeded with the bits of 1.0 in front of the launch
  res_extremes<2, true>(a, A.alpha, lds);
}

// S0 = sum (p + n), S1 = the proximity sum, theta_R = sum |(inf − p) + n|, L = sum log gap + sum log p + sum log n — at the state with
// (p, n) (which = 0) or at the trial point with (pt, nt) (which = 1); x, s, c are the caller's vectors of that point either way
extern "C" __global__ __launch_bounds__(256) void resto_merit(const RestoArgs A) {
  __shared__ double lds[21];
  const long long stride = (long long)gridDim.x * 256;
  const double *P = A.which ? A.pt : A.p, *N = A.which ? A.nt : A.n_;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const unsigned f = A.fx[i];
      const double x = A.x[i];
      const double d = x - A.xR[i];
      v[1] += A.wx[i] * (d * d);
      if (f & 1) v[3] += log(x - A.xl[i]);
      if (f & 2) v[3] += log(A.xu[i] - x);
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      double inf;
      if (f & 4) {
        inf = A.c[j] - A.ceq[j];
      } else {
        const double s = A.s[j];
        inf = A.c[j] - s;
        const double d = s - A.sR[j];
        v[1] += A.ws[j] * (d * d);
        if (f & 1) v[3] += log(s - A.rl[j]);
        if (f & 2) v[3] += log(A.ru[j] - s);
      }
      const double p = P[j], n = N[j];
      v[0] += p + n;
      v[2] += res_abs((inf - p) + n);
      v[3] += log(p);
      v[3] += log(n);
    }
  }
  if (!res_sums<4>(A, v, lds)) return;
  if (threadIdx.x == 0) {
    A.out[0] = A.rho * lds[0] + (0.5 * A.zeta) * lds[1];
    A.out[1] = lds[2];
    A.out[2] = lds[3];
  }
}

// the slope of the restoration's barrier objective along the direction, and the INNER block of a new search — word for word what
// search_begin leaves
extern "C" __global__ __launch_bounds__(256) void resto_begin(const RestoArgs A) {
  __shared__ double lds[21];
  const long long stride = (long long)gridDim.x * 256;
  const double mu = A.mu, zeta = A.zeta, rho = A.rho;
  double v[1] = {0.0};      // the slope: the terms of this lane in index order
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const bool hl = A.fx[i] & 1, hu = A.fx[i] & 2;
      const double x = A.x[i];
      double ml = 0.0, mu_u = 0.0;
      if (hl) { const double d = x - A.xl[i]; ml = mu / d; }
      if (hu) { const double d = A.xu[i] - x; mu_u = mu / d; }
      const double zw = zeta * A.wx[i];
      const double gx = (mu_u - ml) + zw * (x - A.xR[i]);
      v[0] += gx * A.sol[i];
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      if (!(f & 4)) {
        const double s = A.s[j];
        double ml = 0.0, mu_u = 0.0;
        if (f & 1) { const double e = s - A.rl[j]; ml = mu / e; }
        if (f & 2) { const double e = A.ru[j] - s; mu_u = mu / e; }
        const double gs = mu_u - ml;
        const double zs = zeta * A.ws[j];
        const double gsr = gs + zs * (s - A.sR[j]);
        v[0] += gsr * A.ds[j];
      }
      const double tp = (rho - mu / A.p[j]) * A.dp[j], tn = (rho - mu / A.n_[j]) * A.dn[j];
      v[0] += tp + tn;
    }
  }
  if (!res_sums<1>(A, v, lds)) return;
  if (threadIdx.x != 0) return;
  double *ctl = A.ictl;
  const double slope = lds[0], amax = __longlong_as_double((long long)A.alpha[0]), theta0 = A.merit0[1];
  const bool usable = amax > 0.0 && slope == slope;
  ctl[SW_ALPHA] = usable ? amax : 0.0;
  ctl[SW_ALPHA_MAX] = amax;
  ctl[SW_PHI0] = A.merit0[0] - mu * A.merit0[2];
  ctl[SW_THETA0] = theta0;
  ctl[SW_SLOPE] = slope;
  const long long flags = res_word(ctl, SW_FLAGS);
  if (!(flags & 1)) {
    const double t1 = theta0 > 1.0 ? theta0 : 1.0;
    ctl[SW_THETA_MIN] = 1e-4 * t1;
    ctl[SW_THETA_MAX] = 1e4 * t1;
    res_set_word(ctl, SW_FLAGS, flags | 1);
  }
  res_set_word(ctl, SW_PHI_T, RES_NAN_BITS);      // no trial yet
  res_set_word(ctl, SW_THETA_T, RES_NAN_BITS);
  res_set_word(ctl, SW_STATUS, usable ? RES_SEARCHING : RES_UNUSABLE);
  res_set_word(ctl, SW_TRIALS, 0);
  ctl[13] = 0.0; ctl[14] = 0.0; ctl[15] = 0.0;
}

extern "C" __global__ __launch_bounds__(256) void resto_trial(const RestoArgs A) {
  const long long status = res_word(A.ictl, SW_STATUS);
  if (status == RES_FAILED || status == RES_UNUSABLE) return;      // nothing is stored
  const double alpha = A.ictl[SW_ALPHA];
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      A.xt[i] = A.x[i] + alpha * A.sol[i];
    } else {
      const long long j = i - A.nvar;
      A.pt[j] = A.p[j] + alpha * A.dp[j];
      A.nt[j] = A.n_[j] + alpha * A.dn[j];
      if (A.fc[j] & 4) continue;
      A.st[j] = A.s[j] + alpha * A.ds[j];
    }
  }
}

extern "C" __global__ __launch_bounds__(256) void resto_update(const RestoArgs A) {
  const long long stride = (long long)gridDim.x * 256;
  const double ap = __longlong_as_double((long long)A.alpha[0]), ad = __longlong_as_double((long long)A.alpha[1]);
  if (!(ap > 0.0) || !(ad > 0.0)) return;      // a step length of +0.0: the state or the direction was unusable — nothing moves
  const double mu = A.mu, kappa = A.kappa;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const unsigned f = A.fx[i];
      const double x = A.x[i] + ap * A.sol[i];
      A.x[i] = x;
      if (f & 1) A.zL[i] = res_guard(A.zL[i] + ad * A.dzL[i], x - A.xl[i], mu, kappa);
      if (f & 2) A.zU[i] = res_guard(A.zU[i] + ad * A.dzU[i], A.xu[i] - x, mu, kappa);
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      A.y[j] = A.y[j] + ap * A.sol[i];
      const double p = A.p[j] + ap * A.dp[j], n = A.n_[j] + ap * A.dn[j];
      A.p[j] = p;
      A.n_[j] = n;
      A.zp[j] = res_guard(A.zp[j] + ad * A.dzp[j], p, mu, kappa);
      A.zn[j] = res_guard(A.zn[j] + ad * A.dzn[j], n, mu, kappa);
      if (f & 4) continue;
      const double s = A.s[j] + ap * A.ds[j];
      A.s[j] = s;
      if (f & 1) A.vL[j] = res_guard(A.vL[j] + ad * A.dvL[j], s - A.rl[j], mu, kappa);
      if (f & 2) A.vU[j] = res_guard(A.vU[j] + ad * A.dvU[j], A.ru[j] - s, mu, kappa);
    }
  }
}

extern "C" __global__ __launch_bounds__(256) void resto_error(const RestoArgs A) {
  __shared__ double lds[21];
  __shared__ unsigned long long lds_max[4 * (IEM_TILE / IEM_WAVE)];
  const long long stride = (long long)gridDim.x * 256;
  const double mu = A.mu, zeta = A.zeta, rho = A.rho;
  unsigned long long m0 = 0ull, m1 = 0ull, m2 = 0ull, m3 = 0ull;
  double v[4] = {0.0, 0.0, 0.0, 0.0};      // sum |y|, sum of the multipliers, theta_R, L: the last two in resto_merit's order
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const unsigned f = A.fx[i];
      const double x = A.x[i];
      const double zw = zeta * A.wx[i];
      double t = (A.r ? A.r[i] : 0.0) + zw * (x - A.xR[i]);
      if (f & 1) {
        const double d = x - A.xl[i], z = A.zL[i];
        t = t - z;
        m3 = res_umax(m3, res_abs_bits(d * z - mu));
        v[1] += z;
        v[3] += log(d);
      }
      if (f & 2) {
        const double d = A.xu[i] - x, z = A.zU[i];
        t = t + z;
        m3 = res_umax(m3, res_abs_bits(d * z - mu));
        v[1] += z;
        v[3] += log(d);
      }
      m0 = res_umax(m0, res_abs_bits(t));
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      const double y = A.y[j];
      v[0] += res_abs(y);
      double inf;
      if (f & 4) {
        inf = A.c[j] - A.ceq[j];
      } else {
        const double s = A.s[j];
        inf = A.c[j] - s;
        const double zs = zeta * A.ws[j];
        double t = zs * (s - A.sR[j]) - y;
        if (f & 1) {
          const double e = s - A.rl[j], z = A.vL[j];
          t = t - z;
          m3 = res_umax(m3, res_abs_bits(e * z - mu));
          v[1] += z;
          v[3] += log(e);
        }
        if (f & 2) {
          const double e = A.ru[j] - s, z = A.vU[j];
          t = t + z;
          m3 = res_umax(m3, res_abs_bits(e * z - mu));
          v[1] += z;
          v[3] += log(e);
        }
        m1 = res_umax(m1, res_abs_bits(t));
      }
      const double p = A.p[j], n = A.n_[j], zp = A.zp[j], zn = A.zn[j];
      m1 = res_umax(m1, res_abs_bits((rho - y) - zp));
      m1 = res_umax(m1, res_abs_bits((rho + y) - zn));
      const double rc = (inf - p) + n;
      m2 = res_umax(m2, res_abs_bits(rc));
      m3 = res_umax(m3, res_abs_bits(p * zp - mu));
      m3 = res_umax(m3, res_abs_bits(n * zn - mu));
      v[1] += zp;
      v[1] += zn;
      v[2] += res_abs(rc);
      v[3] += log(p);
      v[3] += log(n);
    }
  }
  unsigned long long mx[4] = {A.r ? m0 : 0ull, m1, m2, m3};      // out[0..3] were zeroed in front of the launch
  res_extremes<4, false>(mx, reinterpret_cast<unsigned long long *>(A.out), lds_max);
  if (!res_sums<4>(A, v, lds)) return;
  if (threadIdx.x < 4) A.out[4 + threadIdx.x] = lds[threadIdx.x];
  if (threadIdx.x == 4 && !A.r) A.out[0] = __longlong_as_double(RES_NAN_BITS);      // no r: no dual infeasibility in x
}

// the return test: is the new iterate acceptable to the ORIGINAL filter, and theta small enough against the start of the phase?
extern "C" __global__ __launch_bounds__(64) void resto_check(const RestoArgs A) {
  const int lane = (int)threadIdx.x;
  if (res_word(A.blk, RW_STATE) != RES_ACTIVE) return;      // NONE, or decided already: nothing is written
  const double theta = A.merit[0];
  const double phi = A.f[0] - A.mu * A.merit[1];
  long long count = res_word(A.octl, SW_COUNT);
  count = count < 0 ? 0 : count > A.capacity ? A.capacity : count;
  bool hit = false;
  for (long long k = lane; k < count; k += 64) hit = hit || (theta >= A.ofilter[2 * k] && phi >= A.ofilter[2 * k + 1]);
  const bool dominated = __ballot(hit) != 0ull;
  const bool ok = res_finite(theta) && res_finite(phi) && theta <= A.kappa_resto * A.blk[RW_THETA_START] && theta <= A.octl[SW_THETA_MAX] && !dominated;
  if (lane == 0) {
    A.blk[RW_THETA] = theta;
    A.blk[RW_PHI] = phi;
    if (ok) res_set_word(A.blk, RW_STATE, RES_RETURN);
  }
}

// the integer maximum of the present bound multipliers into word RW_ZMAX of the block (zeroed in front of the launch)
extern "C" __global__ __launch_bounds__(256) void resto_leave_max(const RestoArgs A) {
  __shared__ unsigned long long lds[IEM_TILE / IEM_WAVE];
  const long long stride = (long long)gridDim.x * 256;
  unsigned long long m = 0ull;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const unsigned f = A.fx[i];
      if (f & 1) m = res_umax(m, res_abs_bits(A.zL[i]));
      if (f & 2) m = res_umax(m, res_abs_bits(A.zU[i]));
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      if (f & 4) continue;
      if (f & 1) m = res_umax(m, res_abs_bits(A.vL[j]));
      if (f & 2) m = res_umax(m, res_abs_bits(A.vU[j]));
    }
  }
  unsigned long long a[1] = {m};
  res_extremes<1, false>(a, reinterpret_cast<unsigned long long *>(A.blk + RW_ZMAX), lds);
}

extern "C" __global__ __launch_bounds__(256) void resto_leave(const RestoArgs A) {
  const long long stride = (long long)gridDim.x * 256;
  const bool reset = A.blk[RW_ZMAX] > A.threshold || A.blk[RW_ZMAX] != A.blk[RW_ZMAX];      // (a NaN multiplier resets them too)
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      if (!reset) continue;
      const unsigned f = A.fx[i];
      if (f & 1) A.zL[i] = 1.0;
      if (f & 2) A.zU[i] = 1.0;
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      A.y[j] = 0.0;
      if ((f & 4) || !reset) continue;
      if (f & 1) A.vL[j] = 1.0;
      if (f & 2) A.vU[j] = 1.0;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) res_set_word(A.blk, RW_STATE, RES_NONE);
}
