// i7m_timeline.h — per-wave timeline records for the -DI7M_DIAG library only (tools/timeline.py):
// each instrumented kernel's waves record [start, end] (s_memrealtime, the 100 MHz device-wide
// clock), the hardware slot they ran on (HW_ID, XCC_ID) and the kernel / workgroup, so a tool can
// see how a launch's waves were spread over the 1024 SIMDs and how much of the launch each SIMD
// sat idle (load imbalance, tails); and cycle stamps inside one ADMM kernel (I7M_STAMP,
// tl_write_stamps; tools/step_stamps.py).  The release library compiles I7M_TL and I7M_STAMP to
// nothing.
//
// Buffer layout (device, u64): [0] unused, [1] capacity (records), [2..7] unused, then 4 u64 per
// record: t_start, t_end, HW_ID | XCC_ID << 32, kernel id | workgroup << 8.  Record slot =
// kernel id << 16 | wave index in the grid: no atomics (a counter shared by every wave serialised
// the waves' exits and stretched a B = 4096 launch 3x), so a buffer holds one launch per kernel —
// the tool runs a single SQP iteration.
#pragma once

#include <hip/hip_runtime.h>

#ifdef I7M_DIAG
namespace i7m {

// one copy per translation unit (no -fgpu-rdc): each unit exports its own setter
static __device__ unsigned long long* g_tl = nullptr;

struct TlScope {
  unsigned long long t0;
  int kid;
  __device__ __forceinline__ explicit TlScope(int k) : kid(k) { t0 = __builtin_amdgcn_s_memrealtime(); }
  __device__ __forceinline__ ~TlScope() {
    unsigned long long* tl = g_tl;
    if (tl && (threadIdx.x & 63) == 0) {
      const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
      // s_getreg: HW_ID (id 4) and XCC_ID (id 20), all 32 bits
      const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);
      const unsigned xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
      const unsigned long long wv = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
      const unsigned long long i = ((unsigned long long)kid << 16) + wv;
      if (wv < (1ULL << 16) && i < tl[1]) {  // (a launch of more than 65536 waves records its first 65536)
        unsigned long long* r = tl + 8 + 4 * i;
        r[0] = t0;
        r[1] = t1;
        r[2] = (unsigned long long)hw | ((unsigned long long)xcc << 32);
        r[3] = (unsigned long long)kid | ((unsigned long long)blockIdx.x << 8);
      }
    }
  }
};

// host side: point this unit's kernels at a record buffer (nullptr: off)
static inline int tl_set(void* p) {
  unsigned long long* v = static_cast<unsigned long long*>(p);
  return hipMemcpyToSymbol(HIP_SYMBOL(g_tl), &v, sizeof(v)) == hipSuccess ? 0 : -1;
}

// Cycle stamps inside one kernel (tools/step_stamps.py): s_memtime (the shader clock) between
// sched barriers, waited for, kept in `arr[i]` when `on`.  The stamps fence the schedule and drain
// LDS reads: read the shares, not the length.
#define I7M_STAMP(arr, i, on)                                                   \
  do {                                                                          \
    __builtin_amdgcn_sched_barrier(0);                                          \
    unsigned long long v_;                                                      \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v_)::"memory"); \
    __builtin_amdgcn_sched_barrier(0);                                          \
    if (on) (arr)[i] = v_;                                                      \
  } while (0)
// ... written by one lane to record area 5 (kernel id 5's first slots): r[0..8] the stamps (zero
// past the n taken), r[9] the I7M_ABLATE tag, r[10] the layout: 0 the streaming OSQP iteration
// kernels, 1 the resident one, 2 the factor, 3 the scaling.
__device__ __forceinline__ void tl_write_stamps(const unsigned long long* stamps, int n, int ablate, int layout) {
  if (!g_tl) return;
  unsigned long long* r = g_tl + 8 + 4 * (5ull << 16);
  for (int i = 0; i < 9; ++i) r[i] = i < n ? stamps[i] : 0;
  r[9] = (unsigned long long)ablate;
  r[10] = (unsigned long long)layout;
}

}  // namespace i7m
#define I7M_TL(kid) i7m::TlScope i7m_tl_scope_(kid)
#else
#define I7M_TL(kid)
#define I7M_STAMP(arr, i, on)
#endif
