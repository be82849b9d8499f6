// iem_kkt_residual_device.h — the finishing kernels of iem_kkt_residual / iem_kkt_solve_refined (a code object of its own: no
// other source key knows of it).  Compiled with -ffp-contract=off: every line below is the order of operations of the contract
// in include/iem.h.
//
//   kkt_residual:  p = K0·sol from iem_kktprod (K0 = [W, J'; J, 0]), then per entry
//                    i <  nvar:  r = rhs − (p + (sigma + delta_w)·sol)
//                    i >= nvar:  r = rhs − (p − delta_c·sol)
//                  and, where asked for, max |r| into *norm: the bit pattern of a non-negative double orders as an unsigned 64-bit
//                  integer (a NaN's lies above every finite one), so the maximum is taken on the patterns — per lane, across the
//                  wave by shuffles, across waves by ONE integer atomicMax per wave.  No float atomic, no order dependence: the
//                  result is bitwise reproducible.  *norm is zeroed by the runtime in front of the launch.
//   kkt_axpy1:     sol += d (one rounded add per entry, what the host loop's vector add does)
//
// One thread takes the entries i, i + stride, ...: plain vector loads and stores.

struct KktResidualArgs {
  const double *p, *rhs, *sol, *sigma;   // sigma: nvar entries or null
  double *r;
  unsigned long long *norm;              // null: no norm
  double dw, dc;
  long long nvar, n;                     // n = nvar + ncon
};

extern "C" __global__ __launch_bounds__(256) void kkt_residual(const KktResidualArgs A) {
  const long long stride = (long long)gridDim.x * 256;
  unsigned long long best = 0ull;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    const double s = A.sol[i];
    double t;
    if (i < A.nvar) {
      const double d = (A.sigma ? A.sigma[i] : 0.0) + A.dw;
      t = A.p[i] + d * s;
    } else {
      t = A.p[i] - A.dc * s;
    }
    const double r = A.rhs[i] - t;
    A.r[i] = r;
    const unsigned long long b = (unsigned long long)__double_as_longlong(r) & 0x7fffffffffffffffull;   // |r|
    best = b > best ? b : best;
  }
  if (!A.norm) return;
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o, 64);
    best = other > best ? other : best;
  }
  if ((threadIdx.x & 63) == 0 && best) atomicMax(A.norm, best);
}

struct KktAxpyArgs {
  double *sol;
  const double *d;
  long long n;
};

extern "C" __global__ __launch_bounds__(256) void kkt_axpy1(const KktAxpyArgs A) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) A.sol[i] = A.sol[i] + A.d[i];
}
