// iem_barrier_device.h — the kernels of the iem_barrier object (include/iem.h): the algebra of a primal-dual interior-point
// iteration between the evaluation calls and the KKT solver object — the barrier diagonal, the condensed right-hand side, the slack
// and bound-multiplier directions, the fraction-to-the-boundary step lengths, the update with the multiplier safeguard, Ipopt's
// error terms and the two merit sums.  A code object of its own (no other source key knows of it), compiled with
// -ffp-contract=off behind the helpers of iem_device.h (everything in front of its own kernels, with IEM_TILE = 256): every line below is the order of operations
// of the contract in include/iem.h, each operation rounded once.
//
// NO FLOAT ATOMIC in this file: the only atomics are integer atomicMin (barrier_step) and atomicMax (barrier_error) on the bit
// pattern of a non-negative double, which orders like the double itself (the scheme of kkt_residual_dm) — at most ONE per workgroup
// and slot: the waves' values meet in LDS first, and a workgroup whose value cannot change the slot (a relaxed look at it) issues
// none (thousands of same-address atomics serialise in the L2; DESIGN.md 7 f4b has what one atomic per wave cost).  The four
// sums of barrier_error and the two of barrier_merit go through iem_shared_park / iem_shared_last / iem_shared_totals of
// iem_device.h as they stand: every workgroup parks its four values, reduced in a fixed order; the workgroup that arrives last
// totals each column in a fixed order and writes the 8-byte results with plain stores — bitwise reproducible, one launch.  (The
// helpers of iem_device.h that do contain a float atomicAdd — iem_grad_atomic, iem_grad_wave_uniform — are never called here:
// search this file for "atomic".)
//
// One thread takes the entries i, i + stride, ... of [0, nvar + ncon): i < nvar is variable i, otherwise row j = i − nvar.  Plain
// vector loads and stores.  Flags: fx[i] bit 0 = lower bound present, bit 1 = upper; fc[j] the same for an inequality row's slack,
// bit 2 = equality row.  Entries of the slack-side vectors on equality rows are neither read nor written, a multiplier is read
// only where its bound is present, and an absent bound contributes an exact +0.0 (a branch, never a division by infinity).

#define BAR_ONE_BITS 0x3ff0000000000000ull   // 1.0

struct BarrierArgs {
  const double *xl, *xu, *rl, *ru, *ceq;          // relaxed bounds (nvar, nvar, ncon, ncon) and the equality rows' right-hand side (ncon)
  const unsigned char *fx, *fc;
  double *x, *s, *y, *zL, *zU, *vL, *vU;          // the state (barrier_start / barrier_update write it, the others read it)
  const double *r, *c, *sol;                      // sigma grad f + J'y (nvar, may be null in barrier_error), c(x) (ncon), [dx; dy]
  double *ds, *dzL, *dzU, *dvL, *dvU;             // the directions (barrier_step writes, barrier_update reads)
  double *sigma, *dcon, *rhs;                     // barrier_terms
  unsigned long long *alpha;                      // {alpha_primal, alpha_dual} as bit patterns
  double *out;                                    // barrier_error: 8, barrier_merit: 2
  double *red;                                    // 4 n_wg parked values, then the ticket words
  const long long *tab;                           // offs[4] | first[4] | count[4] of iem_shared_totals
  double mu, tau, kappa, push, frac;
  long long nvar, n, n_wg;
};

// torch.maximum / torch.minimum: a NaN in either operand gives a NaN
__device__ __forceinline__ double bar_max(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double bar_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double bar_abs(double a) { return __longlong_as_double(__double_as_longlong(a) & 0x7fffffffffffffffll); }
__device__ __forceinline__ unsigned long long bar_abs_bits(double a) { return (unsigned long long)__double_as_longlong(a) & 0x7fffffffffffffffull; }
// a step-length candidate: its bit pattern, or 0 when it is not > 0 (a NaN, a point on or outside its bound)
__device__ __forceinline__ unsigned long long bar_cand(double a) { return a > 0.0 ? (unsigned long long)__double_as_longlong(a) : 0ull; }
__device__ __forceinline__ unsigned long long bar_umin(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned long long bar_umax(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// The extremes of the workgroup into their slots: per wave by shuffles, across the waves through LDS (NV·4 words), then thread s < NV
// holds value s of the workgroup and issues ONE integer atomic — and none where a relaxed agent-scope look at the slot shows that it
// would not change it (the slot only ever moves towards the extreme, so a stale look can only cost an atomic, never lose a value).
template <int NV, bool IS_MIN>
__device__ __forceinline__ void bar_extremes(unsigned long long (&v)[NV], unsigned long long *slots, unsigned long long *lds) {
  constexpr int NW = IEM_TILE / IEM_WAVE;
#pragma unroll
  for (int s = 0; s < NV; ++s) {
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(v[s], o, 64);
      v[s] = IS_MIN ? bar_umin(v[s], other) : bar_umax(v[s], other);
    }
    if (iem_lane() == 0) lds[iem_wave() * NV + s] = v[s];
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int s = (int)threadIdx.x;
    unsigned long long b = lds[s];
    for (int w = 1; w < NW; ++w) b = IS_MIN ? bar_umin(b, lds[w * NV + s]) : bar_umax(b, lds[w * NV + s]);
    const unsigned long long cur = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (IS_MIN) { if (b < cur) atomicMin(slots + s, b); }
    else if (b > cur) atomicMax(slots + s, b);
  }
}

// Ipopt's projection into the interior (bound_push k1, bound_frac k2)
__device__ __forceinline__ double bar_push(double v, double lo, double hi, bool has_lo, bool has_hi, double k1, double k2) {
  const bool both = has_lo && has_hi;
  if (has_lo) {
    double pl = k1 * bar_max(bar_abs(lo), 1.0);
    if (both) pl = bar_min(pl, k2 * (hi - lo));
    v = bar_max(v, lo + pl);
  }
  if (has_hi) {
    double pu = k1 * bar_max(bar_abs(hi), 1.0);
    if (both) pu = bar_min(pu, k2 * (hi - lo));
    v = bar_min(v, hi - pu);
  }
  return v;
}

extern "C" __global__ __launch_bounds__(256) void barrier_start(const BarrierArgs A) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const bool hl = A.fx[i] & 1, hu = A.fx[i] & 2;
      if (hl || hu) A.x[i] = bar_push(A.x[i], A.xl[i], A.xu[i], hl, hu, A.push, A.frac);
      A.zL[i] = hl ? 1.0 : 0.0;
      A.zU[i] = hu ? 1.0 : 0.0;
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      if (f & 4) continue;
      const bool gl = f & 1, gu = f & 2;
      A.s[j] = bar_push(A.c[j], A.rl[j], A.ru[j], gl, gu, A.push, A.frac);
      A.vL[j] = gl ? 1.0 : 0.0;
      A.vU[j] = gu ? 1.0 : 0.0;
    }
  }
}

extern "C" __global__ __launch_bounds__(256) void barrier_terms(const BarrierArgs A) {
  const long long stride = (long long)gridDim.x * 256;
  const double mu = A.mu;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const bool hl = A.fx[i] & 1, hu = A.fx[i] & 2;
      const double x = A.x[i];
      double sl = 0.0, su = 0.0, ml = 0.0, mu_u = 0.0;
      if (hl) { const double d = x - A.xl[i]; sl = A.zL[i] / d; ml = mu / d; }
      if (hu) { const double d = A.xu[i] - x; su = A.zU[i] / d; mu_u = mu / d; }
      A.sigma[i] = sl + su;
      const double gb = mu_u - ml;
      A.rhs[i] = -(A.r[i] + gb);
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      if (f & 4) {
        A.dcon[j] = 0.0;
        A.rhs[i] = -(A.c[j] - A.ceq[j]);
        continue;
      }
      const double s = A.s[j];
      double sl = 0.0, su = 0.0, ml = 0.0, mu_u = 0.0;
      if (f & 1) { const double e = s - A.rl[j]; sl = A.vL[j] / e; ml = mu / e; }
      if (f & 2) { const double e = A.ru[j] - s; su = A.vU[j] / e; mu_u = mu / e; }
      const double sigs = sl + su, gs = mu_u - ml;
      const double rs = gs - A.y[j], inv = 1.0 / sigs;
      A.dcon[j] = inv;
      A.rhs[i] = -((A.c[j] - s) + rs * inv);
    }
  }
}

extern "C" __global__ __launch_bounds__(256) void barrier_step(const BarrierArgs A) {
  __shared__ unsigned long long lds[2 * (IEM_TILE / IEM_WAVE)];
  const long long stride = (long long)gridDim.x * 256;
  const double mu = A.mu, tau = A.tau, ntau = -A.tau;
  unsigned long long ap = BAR_ONE_BITS, ad = BAR_ONE_BITS;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const bool hl = A.fx[i] & 1, hu = A.fx[i] & 2;
      const double x = A.x[i], dx = A.sol[i];
      double dzl = 0.0, dzu = 0.0;
      if (dx != dx) ap = 0ull;      // a NaN in the direction: unusable, whatever the bounds
      if (hl) {
        const double d = x - A.xl[i], z = A.zL[i];
        dzl = (mu / d - z) - (z / d) * dx;
        if (dx < 0.0) ap = bar_umin(ap, bar_cand((ntau * d) / dx));
        if (dzl < 0.0) ad = bar_umin(ad, bar_cand((ntau * z) / dzl));
        if (dzl != dzl) ad = 0ull;
      }
      if (hu) {
        const double d = A.xu[i] - x, z = A.zU[i];
        dzu = (mu / d - z) + (z / d) * dx;
        if (dx > 0.0) ap = bar_umin(ap, bar_cand((tau * d) / dx));
        if (dzu < 0.0) ad = bar_umin(ad, bar_cand((ntau * z) / dzu));
        if (dzu != dzu) ad = 0ull;
      }
      A.dzL[i] = dzl;
      A.dzU[i] = dzu;
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      if (A.sol[i] != A.sol[i]) ap = 0ull;      // dy
      if (f & 4) continue;
      const bool gl = f & 1, gu = f & 2;
      const double s = A.s[j];
      double el = 0.0, eu = 0.0, vl = 0.0, vu = 0.0, sl = 0.0, su = 0.0, ml = 0.0, mu_u = 0.0;
      if (gl) { el = s - A.rl[j]; vl = A.vL[j]; sl = vl / el; ml = mu / el; }
      if (gu) { eu = A.ru[j] - s; vu = A.vU[j]; su = vu / eu; mu_u = mu / eu; }
      const double sigs = sl + su, gs = mu_u - ml;
      const double rs = gs - A.y[j];
      const double ds = (A.sol[i] - rs) / sigs;
      A.ds[j] = ds;
      if (ds != ds) ap = 0ull;
      double dvl = 0.0, dvu = 0.0;
      if (gl) {
        dvl = (ml - vl) - sl * ds;
        if (ds < 0.0) ap = bar_umin(ap, bar_cand((ntau * el) / ds));
        if (dvl < 0.0) ad = bar_umin(ad, bar_cand((ntau * vl) / dvl));
        if (dvl != dvl) ad = 0ull;
      }
      if (gu) {
        dvu = (mu_u - vu) + su * ds;
        if (ds > 0.0) ap = bar_umin(ap, bar_cand((tau * eu) / ds));
        if (dvu < 0.0) ad = bar_umin(ad, bar_cand((ntau * vu) / dvu));
        if (dvu != dvu) ad = 0ull;
      }
      A.dvL[j] = dvl;
      A.dvU[j] = dvu;
    }
  }
  unsigned long long a[2] = {ap, ad};      // the slots were seeded with the bits of 1.0 in front of the launch
  bar_extremes<2, true>(a, A.alpha, lds);
}

// the safeguard of Ipopt's eq. (16):  z = min(max(z, mu / (kappa gap)), (kappa mu) / gap)
__device__ __forceinline__ double bar_guard(double z, double gap, double mu, double kappa) {
  return bar_min(bar_max(z, mu / (kappa * gap)), (kappa * mu) / gap);
}

extern "C" __global__ __launch_bounds__(256) void barrier_update(const BarrierArgs A) {
  const long long stride = (long long)gridDim.x * 256;
  const double ap = __longlong_as_double((long long)A.alpha[0]), ad = __longlong_as_double((long long)A.alpha[1]);
  if (!(ap > 0.0) || !(ad > 0.0)) return;      // a step length of +0.0: the state or the direction was unusable — nothing moves
  const double mu = A.mu, kappa = A.kappa;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const unsigned f = A.fx[i];
      const double x = A.x[i] + ap * A.sol[i];
      A.x[i] = x;
      if (f & 1) A.zL[i] = bar_guard(A.zL[i] + ad * A.dzL[i], x - A.xl[i], mu, kappa);
      if (f & 2) A.zU[i] = bar_guard(A.zU[i] + ad * A.dzU[i], A.xu[i] - x, mu, kappa);
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      A.y[j] = A.y[j] + ap * A.sol[i];
      if (f & 4) continue;
      const double s = A.s[j] + ap * A.ds[j];
      A.s[j] = s;
      if (f & 1) A.vL[j] = bar_guard(A.vL[j] + ad * A.dvL[j], s - A.rl[j], mu, kappa);
      if (f & 2) A.vU[j] = bar_guard(A.vU[j] + ad * A.dvU[j], A.ru[j] - s, mu, kappa);
    }
  }
}

// the four sums of the launch: parked per workgroup, totalled by the workgroup that arrives last (lds: 4 (NW + 1) + 1 doubles)
template <int NV>
__device__ __forceinline__ bool bar_sums(const BarrierArgs &A, const double (&v)[NV], double *lds) {
  iem_shared_park<NV>(v, A.red, A.tab, (long long)blockIdx.x, lds);
  if (!iem_shared_last(A.red + 4 * A.n_wg, (long long)blockIdx.x, A.n_wg, lds + 20)) return false;
  iem_shared_totals(NV, A.red, A.tab, A.tab + 4, A.tab + 8, lds);
  return true;
}

extern "C" __global__ __launch_bounds__(256) void barrier_error(const BarrierArgs A) {
  __shared__ double lds[21];
  __shared__ unsigned long long lds_max[4 * (IEM_TILE / IEM_WAVE)];
  const long long stride = (long long)gridDim.x * 256;
  const double mu = A.mu;
  unsigned long long m0 = 0ull, m1 = 0ull, m2 = 0ull, m3 = 0ull;
  double v[4] = {0.0, 0.0, 0.0, 0.0};      // sum |y|, sum of the present multipliers, theta, sum log gap
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const unsigned f = A.fx[i];
      const double x = A.x[i];
      double t = A.r ? A.r[i] : 0.0;
      if (f & 1) {
        const double d = x - A.xl[i], z = A.zL[i];
        t = t - z;
        m3 = bar_umax(m3, bar_abs_bits(d * z - mu));
        v[1] += z;
        v[3] += log(d);
      }
      if (f & 2) {
        const double d = A.xu[i] - x, z = A.zU[i];
        t = t + z;
        m3 = bar_umax(m3, bar_abs_bits(d * z - mu));
        v[1] += z;
        v[3] += log(d);
      }
      m0 = bar_umax(m0, bar_abs_bits(t));
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      const double y = A.y[j];
      v[0] += bar_abs(y);
      double inf;
      if (f & 4) {
        inf = A.c[j] - A.ceq[j];
      } else {
        const double s = A.s[j];
        inf = A.c[j] - s;
        double t = -y;
        if (f & 1) {
          const double e = s - A.rl[j], z = A.vL[j];
          t = t - z;
          m3 = bar_umax(m3, bar_abs_bits(e * z - mu));
          v[1] += z;
          v[3] += log(e);
        }
        if (f & 2) {
          const double e = A.ru[j] - s, z = A.vU[j];
          t = t + z;
          m3 = bar_umax(m3, bar_abs_bits(e * z - mu));
          v[1] += z;
          v[3] += log(e);
        }
        m1 = bar_umax(m1, bar_abs_bits(t));
      }
      m2 = bar_umax(m2, bar_abs_bits(inf));
      v[2] += bar_abs(inf);
    }
  }
  unsigned long long mx[4] = {A.r ? m0 : 0ull, m1, m2, m3};      // out[0..3] were zeroed in front of the launch
  bar_extremes<4, false>(mx, reinterpret_cast<unsigned long long *>(A.out), lds_max);
  if (!bar_sums<4>(A, v, lds)) return;
  if (threadIdx.x < 4) A.out[4 + threadIdx.x] = lds[threadIdx.x];
  if (threadIdx.x == 4 && !A.r) A.out[0] = __longlong_as_double(0x7ff8000000000000ll);      // no r: no dual infeasibility in x
}

extern "C" __global__ __launch_bounds__(256) void barrier_merit(const BarrierArgs A) {
  __shared__ double lds[21];
  const long long stride = (long long)gridDim.x * 256;
  double v[2] = {0.0, 0.0};      // theta, sum log gap: the accumulation order of barrier_error's v[2], v[3]
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const unsigned f = A.fx[i];
      const double x = A.x[i];
      if (f & 1) v[1] += log(x - A.xl[i]);
      if (f & 2) v[1] += log(A.xu[i] - x);
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      double inf;
      if (f & 4) {
        inf = A.c[j] - A.ceq[j];
      } else {
        const double s = A.s[j];
        inf = A.c[j] - s;
        if (f & 1) v[1] += log(s - A.rl[j]);
        if (f & 2) v[1] += log(A.ru[j] - s);
      }
      v[0] += bar_abs(inf);
    }
  }
  if (!bar_sums<2>(A, v, lds)) return;
  if (threadIdx.x < 2) A.out[threadIdx.x] = lds[threadIdx.x];
}
