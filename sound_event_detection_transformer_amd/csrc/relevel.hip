// relevel.hip - the level of E regions of a staged sound bank measured on the device, and the gain that brings each to its target
// written into the DEVICE records of the event (SedtScapeEvent) and of its reverberation tail (SedtReverbTail) before they are mixed
// (utilities/relevel.py; DESIGN.md section 4, "Levels measured after the effects"; tests/relevel_ref.py restates it in float64).
// The reference has no counterpart: its corpora were mixed offline by a generator that measures every processed event.
//   * relevel_kernel   one workgroup of 256 per job (SedtRelevelJob, include/sedt_hip.h): the region flat[off .. off + n)
//       mode 0 (RMS)      level = (sum of x * x) / n, squares and sums in float64 in sedt_bank_stats' order: thread t adds elements
//                         t, t + 256, ..., then the fixed tree over the 256 partial sums; counts n, 0, 0, 0 (n clamped to 2^31 - 1)
//       mode 1 (BS.1770)  level = zbar, counts = J, n_abs, n_rel, short: loud_measure of loudness_dev.h, the chain of sedt_loudness
//                         on the region - the same coefficients, hop map, hop and absolute gate, the hop energies to the job's own
//                         doubles of the workspace
//     then, by thread 0, g = float32(target / sqrt(level)) from float64 arithmetic: a level that is finite and > 0 gives status 0 and
//     g goes to ev[job.ev].gain and tails[job.tail].gain (an index of -1 is skipped); any other level - a silent region, one under the
//     absolute gate in every block, one with a NaN or infinite sample - gives status 1 and both records keep the gain the host wrote.
// The kernel re-checks its DEVICE record (rl_job_ok) against the bank, both record tables and the workspace before it touches memory:
// a bad record raises status 2 and nothing else is read or written for it.  No atomics, no allocation, no synchronisation: the same
// call gives the same bits.  A record is named by at most one job of a call.
#include "common.h"
#include "loudness_dev.h"

#include <math.h>

namespace sedt {

__host__ __device__ inline long rl_job_doubles(int mode, long n, int hop) { return mode == 1 ? n / hop + 1 : 0; }

// what both the entry point (on the host copies) and the kernel (on the device copies) ask of a job
__host__ __device__ inline bool rl_job_ok(const SedtRelevelJob& j, int mode, int hop, long flat_len, int n_ev, int n_tails, long work_len) {
  if (j.off < 0 || j.n < 1 || j.off > flat_len || j.n > flat_len - j.off) return false;
  if (j.ev < -1 || j.ev >= n_ev || j.tail < -1 || j.tail >= n_tails) return false;
  if (!(j.target > 0.0 && j.target <= 1.7976931348623157e308)) return false;                  // (NaN fails)
  if (j.ws_off < 0 || j.ws_off > work_len || rl_job_doubles(mode, j.n, hop) > work_len - j.ws_off) return false;
  return true;
}

__global__ __launch_bounds__(SEDT_LOUD_THREADS) void relevel_kernel(
    const float* __restrict__ flat, long flat_len, const SedtRelevelJob* __restrict__ jobs, int mode, const double* __restrict__ coef,
    const double* __restrict__ hop_map, int hop, double z_abs, double* __restrict__ work, long work_len, SedtScapeEvent* ev, int n_ev,
    SedtReverbTail* tails, int n_tails, double* __restrict__ level, int32_t* __restrict__ counts, int32_t* __restrict__ status) {
  __shared__ LoudLds lds;
  const int tid = threadIdx.x, e = blockIdx.x;
  const SedtRelevelJob job = jobs[e];
  if (!rl_job_ok(job, mode, hop, flat_len, n_ev, n_tails, work_len)) {      // (uniform over the workgroup)
    if (tid == 0) status[e] = 2;
    return;
  }
  const float* __restrict__ p = flat + job.off;
  double lv;
  long c0, c1 = 0, c2 = 0, c3 = 0;
  if (mode == 1) {
    const LoudResult r = loud_measure(lds, p, (long)job.n, coef, hop_map, hop, z_abs, work + job.ws_off, tid);
    lv = r.zbar, c0 = r.J, c1 = r.n_abs, c2 = r.n_rel, c3 = r.is_short ? 1 : 0;
  } else {
    double a = 0.0;
    for (long i = tid; i < job.n; i += SEDT_LOUD_THREADS) {
      const float x = p[i];
      a = a + (double)x * (double)x;
    }
    lds.sum[tid] = a;
    lds.cnt[tid] = 0;
    loud_tree(lds, tid);
    lv = lds.sum[0] / (double)job.n;
    c0 = (long)job.n;
  }
  if (tid != 0) return;
  level[e] = lv;
  counts[4 * e] = (int32_t)min(c0, 0x7fffffffL);
  counts[4 * e + 1] = (int32_t)min(c1, 0x7fffffffL);
  counts[4 * e + 2] = (int32_t)min(c2, 0x7fffffffL);
  counts[4 * e + 3] = (int32_t)c3;
  if (!(lv > 0.0 && lv <= 1.7976931348623157e308)) {            // silent, under the gate everywhere, or not finite
    status[e] = 1;
    return;
  }
  const float g = (float)(job.target / sqrt(lv));
  if (job.ev >= 0) ev[job.ev].gain = g;
  if (job.tail >= 0) tails[job.tail].gain = g;
  status[e] = 0;
}

// the host half of the entry points: one pass over the HOST copy of the jobs
static int rl_check_jobs(const char* who, const SedtRelevelJob* jobs, int E, int mode, int hop, int64_t flat_len, int n_ev, int n_tails,
                         int64_t* need) {
  int64_t end = 0;
  for (int e = 0; e < E; ++e) {
    const SedtRelevelJob& j = jobs[e];
    SEDT_REQUIRE(j.n >= 1 && j.off >= 0, "%s: job %d is the region off=%lld n=%lld (off >= 0, n >= 1)", who, e, (long long)j.off,
                 (long long)j.n);
    if (flat_len >= 0)
      SEDT_REQUIRE(j.off <= flat_len && j.n <= flat_len - j.off, "%s: job %d (samples %lld .. +%lld) does not lie inside the %lld samples given",
                   who, e, (long long)j.off, (long long)j.n, (long long)flat_len);
    if (n_ev >= 0)
      SEDT_REQUIRE(j.ev >= -1 && j.ev < n_ev && j.tail >= -1 && j.tail < n_tails,
                   "%s: job %d names event record %d of %d and tail record %d of %d (-1: none)", who, e, j.ev, n_ev, j.tail, n_tails);
    SEDT_REQUIRE(j.target > 0.0 && j.target <= 1.7976931348623157e308, "%s: job %d has target=%g: not a finite amplitude > 0", who, e,
                 j.target);
    SEDT_REQUIRE(j.ws_off >= end, "%s: job %d has ws_off=%lld: the regions lie in job order, behind one another (>= %lld)", who, e,
                 (long long)j.ws_off, (long long)end);
    end = j.ws_off + rl_job_doubles(mode, j.n, hop);
  }
  *need = end;
  return 0;
}

}  // namespace sedt

extern "C" int64_t sedt_relevel_workspace(const SedtRelevelJob* jobs_host, int n_jobs, int mode, int hop) {
  using namespace sedt;
  if (!jobs_host || n_jobs < 0 || !(mode == 0 || mode == 1) || hop < 1) {
    set_error("relevel_workspace: null pointer, n_jobs=%d < 0, mode=%d (0: RMS, 1: BS.1770) or hop=%d < 1", n_jobs, mode, hop);
    return -1;
  }
  int64_t need;
  if (rl_check_jobs("relevel_workspace", jobs_host, n_jobs, mode, hop, -1, -1, -1, &need)) return -1;
  return need;
}

extern "C" int sedt_relevel(const float* flat, int64_t flat_len, const SedtRelevelJob* jobs_host, const SedtRelevelJob* jobs_dev, int n_jobs,
                            int mode, const double* coef, const double* hop_map, int hop, double z_abs, double* work, int64_t work_len,
                            SedtScapeEvent* ev, int n_ev, SedtReverbTail* tails, int n_tails, double* level, int32_t* counts,
                            int32_t* status, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(mode == 0 || mode == 1, "relevel: mode=%d (0: RMS, 1: BS.1770)", mode);
  SEDT_REQUIRE(n_jobs >= 0 && flat_len >= 0 && work_len >= 0 && n_ev >= 0 && n_tails >= 0,
               "relevel: n_jobs=%d flat_len=%lld work_len=%lld n_ev=%d n_tails=%d (none may be negative)", n_jobs, (long long)flat_len,
               (long long)work_len, n_ev, n_tails);
  SEDT_REQUIRE(hop >= 1 && z_abs >= 0.0, "relevel: hop=%d (>= 1) z_abs=%g (a number >= 0)", hop, z_abs);
  SEDT_REQUIRE(flat && jobs_host && jobs_dev && level && counts && status && (ev || n_ev == 0) && (tails || n_tails == 0) &&
                   (mode == 0 || (coef && hop_map && work)),
               "relevel: null pointer");
  SEDT_REQUIRE((reinterpret_cast<uintptr_t>(flat) & 3) == 0 && (reinterpret_cast<uintptr_t>(counts) & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(status) & 3) == 0 && (reinterpret_cast<uintptr_t>(jobs_dev) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(ev) & 7) == 0 && (reinterpret_cast<uintptr_t>(tails) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(coef) & 7) == 0 && (reinterpret_cast<uintptr_t>(hop_map) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(work) & 7) == 0 && (reinterpret_cast<uintptr_t>(level) & 7) == 0,
               "relevel: the waveforms, counts and statuses are 4-byte aligned, the records and every float64 buffer 8-byte aligned");
  int64_t need;
  if (rl_check_jobs("relevel", jobs_host, n_jobs, mode, hop, flat_len, n_ev, n_tails, &need)) return 1;
  SEDT_REQUIRE(need <= work_len, "relevel: work_len=%lld is too small: the jobs need %lld doubles (sedt_relevel_workspace)",
               (long long)work_len, (long long)need);
  if (n_jobs == 0) return 0;
  hipLaunchKernelGGL(relevel_kernel, dim3((unsigned)n_jobs), dim3(SEDT_LOUD_THREADS), 0, reinterpret_cast<hipStream_t>(stream), flat,
                     (long)flat_len, jobs_dev, mode, coef, hop_map, hop, z_abs, work, (long)work_len, ev, n_ev, tails, n_tails, level, counts,
                     status);
  return check_launch("relevel");
}
