// iem_halo2_device.h — the TWO-WAY halo exchange and its transpose, for shards of models whose stencils reach to the
// right of their support (forward and central differences: /root/reference/src/transform.jl:535 passes any
// finite-difference method to derivative_expr_data).  Appended to the source behind iem_device.h ONLY for such a shard
// (Options::two_sided, set by iem_create_sharded when reach_right > 0): iem_device.h is part of every model's source, so
// its bytes — and with them the code-object key of every existing model — stay what they were, and a left-reaching
// model keeps running the one-way kernels it always ran.
//
// Second direction of a mailbox: a block of its own BEHIND the one-way layout (word offset B2 = end of the fold data):
//   [B2+0] halo ack (from the left: it consumed what I sent it)   [B2+1, B2+3) halo flags (from the right, per parity)
//   [B2+3] fold ack (from the right)                              [B2+4, B2+6) fold flags (from the left, per parity)
//   [B2+8, ...) halo data [2][NL], then fold data [2][NL]         (NL = doubles one rank sends its LEFT neighbour)
// Sequence numbers are the one-way ones (IEM_MB_HSEQ / IEM_MB_FSEQ): one exchange moves both directions.
// Status bits of the second direction (iem_comm_status): 32 / 64 halo ack / data, 128 / 256 fold ack / data
// (the first direction keeps 1 / 2 and 8 / 16, the all-reduce 4).
#ifndef IEM_HALO2_DEVICE_H
#define IEM_HALO2_DEVICE_H

#define IEM_MB2_HACK 0
#define IEM_MB2_HFLAG 1
#define IEM_MB2_FACK 3
#define IEM_MB2_FFLAG 4
#define IEM_MB2_DATA 8

struct IemHalo2Args : IemHaloArgs {          // src / dst / NH of the base: my LAST reach_left owned supports -> right, front halo entries
  const long long *src_l, *dst_r;            // NL positions each: my FIRST reach_right owned supports -> left, back halo entries
  long long NL, B2;
};

// One workgroup, any size; all sends come before all waits, so no order of the ranks can make two neighbours wait on
// each other.  (a) wait for the acks of both outgoing slots, (b) store both payloads, (c) ONE publish fence, then both
// flags, (d) wait for both incoming flags and copy into the front and back halo entries of x (NaN for what did not
// arrive), (e) ack both.  Every wait is bounded (iem_wait_ge).
__device__ __forceinline__ void iem_halo2_wg(const IemHaloArgs &A0, double *__restrict__ x) {
  const IemHalo2Args &A = static_cast<const IemHalo2Args &>(A0);   // what the host put behind `comm` for a two-sided shard
  const IemCommErr E = {A.mine + IEM_MB_STATUS, A.hstatus, A.ticks};
  const unsigned long long seq = iem_sys_load(A.mine + IEM_MB_HSEQ) + 1;
  const long long par = (long long)(seq & 1);
  const long long nt = (long long)blockDim.x;
  const bool to_r = A.right != nullptr && A.NH > 0, to_l = A.left != nullptr && A.NL > 0;      // what I send
  const bool from_l = A.left != nullptr && A.NH > 0, from_r = A.right != nullptr && A.NL > 0;  // what I receive
  __shared__ int ok2_[2];
  if (threadIdx.x == 0 && seq > 2) {   // the slots of this parity were last used by seq - 2
    if (to_r) iem_wait_ge(A.mine + IEM_MB_HACK, seq - 2, E, 1ULL);
    if (to_l) iem_wait_ge(A.mine + A.B2 + IEM_MB2_HACK, seq - 2, E, 32ULL);
  }
  __syncthreads();
  if (to_r) {
    double *data = reinterpret_cast<double *>(A.right + iem_mb_hdata(A.W, A.G)) + par * A.NH;
    for (long long e = threadIdx.x; e < A.NH; e += nt) iem_sys_stored(data + e, x[A.src[e]]);
  }
  if (to_l) {
    double *data = reinterpret_cast<double *>(A.left + A.B2 + IEM_MB2_DATA) + par * A.NL;
    for (long long e = threadIdx.x; e < A.NL; e += nt) iem_sys_stored(data + e, x[A.src_l[e]]);
  }
  iem_publish_fence();
  if (threadIdx.x == 0) {
    if (to_r) iem_sys_store(A.right + IEM_MB_HFLAG + par, seq);
    if (to_l) iem_sys_store(A.left + A.B2 + IEM_MB2_HFLAG + par, seq);
    ok2_[0] = from_l ? (int)iem_wait_ge(A.mine + IEM_MB_HFLAG + par, seq, E, 2ULL) : 1;
    ok2_[1] = from_r ? (int)iem_wait_ge(A.mine + A.B2 + IEM_MB2_HFLAG + par, seq, E, 64ULL) : 1;
    __threadfence_system();
  }
  __syncthreads();
  if (from_l) {
    const double *data = reinterpret_cast<const double *>(A.mine + iem_mb_hdata(A.W, A.G)) + par * A.NH;
    const int ok = ok2_[0];
    for (long long e = threadIdx.x; e < A.NH; e += nt) x[A.dst[e]] = ok ? iem_sys_loadd(data + e) : __builtin_nan("");   // time-out: poisoned, never stale
  }
  if (from_r) {
    const double *data = reinterpret_cast<const double *>(A.mine + A.B2 + IEM_MB2_DATA) + par * A.NL;
    const int ok = ok2_[1];
    for (long long e = threadIdx.x; e < A.NL; e += nt) x[A.dst_r[e]] = ok ? iem_sys_loadd(data + e) : __builtin_nan("");
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    if (from_l) iem_sys_store(A.left + IEM_MB_HACK, seq);
    if (from_r) iem_sys_store(A.right + A.B2 + IEM_MB2_HACK, seq);
    iem_sys_store(A.mine + IEM_MB_HSEQ, seq);
  }
}
extern "C" __global__ __launch_bounds__(IEM_BLOCK) void iem_halo2_kernel(const IemHalo2Args A) { iem_halo2_wg(A, A.x); }

// The exact transpose, for vectors in VARIABLE space that a transposed operator produced (J'v): my FRONT halo copies hold
// what my rows owe to variables the LEFT neighbour owns, my BACK halo copies what they owe to the RIGHT neighbour's.  Both
// go out and are zeroed here; incoming addends are added to my owned entries in a FIXED order — the left neighbour's
// first, then the right neighbour's — so a shard narrower than reach_left + reach_right (one entry, two addends) still
// sums reproducibly.
struct IemFold2Args {
  double *vec;
  unsigned long long *mine, *left, *right;
  const long long *src, *dst;                // as in IemHalo2Args
  long long NH, W, G, NR;
  unsigned long long *hstatus; long long ticks;
  const long long *src_l, *dst_r;
  long long NL, B2;
};
extern "C" __global__ __launch_bounds__(IEM_BLOCK) void iem_halo2_fold_kernel(const IemFold2Args A) {
  const IemCommErr E = {A.mine + IEM_MB_STATUS, A.hstatus, A.ticks};
  const unsigned long long seq = iem_sys_load(A.mine + IEM_MB_FSEQ) + 1;
  const long long par = (long long)(seq & 1);
  const long long nt = (long long)blockDim.x;
  const bool to_l = A.left != nullptr && A.NH > 0, to_r = A.right != nullptr && A.NL > 0;      // front copies go left, back copies go right
  const bool from_r = A.right != nullptr && A.NH > 0, from_l = A.left != nullptr && A.NL > 0;
  const long long fdata = iem_mb_fdata(A.W, A.G, A.NH, A.NR), fdata2 = A.B2 + IEM_MB2_DATA + 2 * A.NL;
  __shared__ int ok2_[2];
  if (threadIdx.x == 0 && seq > 2) {
    if (to_l) iem_wait_ge(A.mine + IEM_MB_FACK, seq - 2, E, 8ULL);
    if (to_r) iem_wait_ge(A.mine + A.B2 + IEM_MB2_FACK, seq - 2, E, 128ULL);
  }
  __syncthreads();
  if (to_l) {
    double *data = reinterpret_cast<double *>(A.left + fdata) + par * A.NH;
    for (long long e = threadIdx.x; e < A.NH; e += nt) { iem_sys_stored(data + e, A.vec[A.dst[e]]); A.vec[A.dst[e]] = 0.0; }
  }
  if (to_r) {
    double *data = reinterpret_cast<double *>(A.right + fdata2) + par * A.NL;
    for (long long e = threadIdx.x; e < A.NL; e += nt) { iem_sys_stored(data + e, A.vec[A.dst_r[e]]); A.vec[A.dst_r[e]] = 0.0; }
  }
  iem_publish_fence();
  if (threadIdx.x == 0) {
    if (to_l) iem_sys_store(A.left + IEM_MB_FFLAG + par, seq);
    if (to_r) iem_sys_store(A.right + A.B2 + IEM_MB2_FFLAG + par, seq);
    ok2_[0] = from_l ? (int)iem_wait_ge(A.mine + A.B2 + IEM_MB2_FFLAG + par, seq, E, 256ULL) : 1;
    ok2_[1] = from_r ? (int)iem_wait_ge(A.mine + IEM_MB_FFLAG + par, seq, E, 16ULL) : 1;
    __threadfence_system();
  }
  __syncthreads();
  if (from_l) {   // the left neighbour's addends first: into my FIRST reach_right owned supports
    const double *data = reinterpret_cast<const double *>(A.mine + fdata2) + par * A.NL;
    const int ok = ok2_[0];
    for (long long e = threadIdx.x; e < A.NL; e += nt) A.vec[A.src_l[e]] = ok ? A.vec[A.src_l[e]] + iem_sys_loadd(data + e) : __builtin_nan("");
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();   // an entry that takes both addends (narrow shard) is written by two different threads: in this order
  if (from_r) {   // then the right neighbour's: into my LAST reach_left owned supports
    const double *data = reinterpret_cast<const double *>(A.mine + fdata) + par * A.NH;
    const int ok = ok2_[1];
    for (long long e = threadIdx.x; e < A.NH; e += nt) A.vec[A.src[e]] = ok ? A.vec[A.src[e]] + iem_sys_loadd(data + e) : __builtin_nan("");
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    if (from_r) iem_sys_store(A.right + IEM_MB_FACK, seq);
    if (from_l) iem_sys_store(A.left + A.B2 + IEM_MB2_FACK, seq);
    iem_sys_store(A.mine + IEM_MB_FSEQ, seq);
  }
}

// The generated kernels' carrier prologue calls iem_halo_wg(*A.comm, x): in a two-sided shard's source that is the
// two-way exchange (the stand-alone one-way kernels above this line keep their own, unused).
#define iem_halo_wg iem_halo2_wg

#endif  // IEM_HALO2_DEVICE_H
