// Host-side LDS and occupancy planners of the launchers: how much dynamic LDS a kernel may
// ask for (lds_dynamic_max, behind CPR_LDS_GUARD in every unit that launches with dynamic
// LDS), and the event-engine kernels' slab and lanes-per-wave plans (ev_kernels.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "kernels.h"

namespace cpr {

// CUs of the device the first caller runs on
static int device_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus <= 0)
      cus = 256;
  }
  return cus;
}

int64_t lds_dynamic_max(const void* kernel) {
  struct Entry {
    const void* k;
    int dev;
    int64_t room;
  };
  static std::mutex mu;
  static std::vector<Entry> cache;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(mu);
  for (const Entry& e : cache)
    if (e.k == kernel && e.dev == dev) return e.room;
  int lds = 0;
  if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess ||
      lds <= 0)
    lds = 64 * 1024;
  hipFuncAttributes fa{};
  if (hipFuncGetAttributes(&fa, kernel) != hipSuccess) {
    (void)hipGetLastError();
    return 0;  // unknown: no dynamic LDS (not cached, asked again next time)
  }
  const int64_t room = std::max<int64_t>(0, (int64_t)lds - (int64_t)fa.sharedSizeBytes);
  cache.push_back(Entry{kernel, dev, room});
  return room;
}

// envs per wave of a lockstep rollout of n envs on `kernel`: the widest of 64 / 32 / 16 whose
// waves fit the kernel's resident waves per SIMD (occupancy query), so that a small batch
// still runs several waves per SIMD, which hide each other's dependent loads (BASELINE
// configs[4], 65,536 B_k envs: one wave per SIMD at 64; 32 per wave +5.6 % env-steps/s,
// 16 per wave at the 4-wave budget of k_bk_rollout +3.7 % more;
// profiles/r05f_lpw.log, profiles/r05g_lpw.log). CPR_ROLL_LPW overrides it.
int32_t rollout_lanes_per_wave(int64_t n, const void* kernel) {
  const int cus = device_cus();
  if (const char* v = getenv("CPR_ROLL_LPW")) {
    const int32_t w = atoi(v);
    if (w >= 1 && w <= 64) return w;
  }
  int per_cu = 0;  // workgroups of kBlock / 64 waves, i.e. waves per SIMD
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, 0) != hipSuccess ||
      per_cu <= 0) {
    (void)hipGetLastError();
    per_cu = 1;
  }
  const int64_t simds = (int64_t)cus * 4;
  for (int32_t w : {16, 32})
    if ((n + w * simds - 1) / (w * simds) <= per_cu) return w;
  return 64;
}

// lanes per wave that run episodes in the fused event-engine kernels that take the parameter
// (Tailstorm's; the others idle): 64 (CPR_EV_LPW overrides it for A/B runs: 32 with an
// occupancy variant runs the same lanes as twice the waves)
int32_t event_lanes_per_wave() {
  if (const char* v = getenv("CPR_EV_LPW")) {
    const int32_t w = atoi(v);
    if (w >= 1 && w <= 64) return w;
  }
  return 64;
}

// an event-engine kernel's slab for a grid of `blocks` workgroups: the LDS a workgroup gets
// when the grid spreads over the device's CUs (160 KiB per CU), less the kernel's static
// LDS. First the visibility rows of the newest vw vertices (BkMem.vl / TsMem.vl; 64, else
// 32, when they take at most a third of the workgroup's share; CPR_EV_VWIN overrides it,
// 0 = none), then the heap's first kl nodes from what is left, at most 32 (the gym's
// windows hold 14-30 live events; CPR_EV_SLAB overrides it for A/B runs, 0 = every node in
// HBM)
EvSlab ev_slab_plan(int64_t blocks, const void* kernel, int32_t n, int32_t lanes,
                    int32_t trec_rows) {
  if (lanes <= 0) lanes = kBlock;
  const int cus = device_cus();
  const int64_t per_cu = std::max<int64_t>(1, (blocks + cus - 1) / cus);
  // 160 KiB less the kernel's static LDS (reserved as at least 2 KiB, the plans' rule)
  const int64_t room = std::min<int64_t>(lds_dynamic_max(kernel), 160 * 1024 - 2048);
  const int64_t avail = std::min<int64_t>(room, (160 * 1024) / per_cu - (160 * 1024 - room));
  int32_t vw = 0;
  for (int32_t w : {64, 32})
    if (vw == 0 && (int64_t)w * n * lanes * 3 <= avail) vw = w;
  if (const char* v = getenv("CPR_EV_VWIN")) {
    const int32_t w = atoi(v);
    vw = (w >= 1 && (w & (w - 1)) == 0 && w <= 256) ? w : 0;
  }
  int64_t rest = avail - (int64_t)vw * n * lanes;
  if (rest < 0) {
    vw = 0;
    rest = avail;
  }
  // the list-record window (after the visibility rows, 16-aligned; a 16-byte record per row
  // and lane) takes its share before the heap nodes
  int32_t tw = trec_rows > 0 && (trec_rows & (trec_rows - 1)) == 0 ? trec_rows : 0;
  while (tw > 0 && rest - 16 - (int64_t)tw * 16 * lanes < 0) tw >>= 1;
  if (tw > 0) rest -= 16 + (int64_t)tw * 16 * lanes;
  int32_t kl = (int32_t)std::min<int64_t>(32, std::max<int64_t>(0, rest / (lanes * 24)));
  if (const char* v = getenv("CPR_EV_SLAB")) kl = std::max(0, std::min(32, atoi(v)));
  auto layout = [&](EvSlab& s) {
    const size_t vis_end = (size_t)s.kl * lanes * 24 + (size_t)s.vw * n * lanes;
    s.tw_off = (vis_end + 15) / 16 * 16;
    s.bytes = s.tw > 0 ? s.tw_off + (size_t)s.tw * 16 * lanes : vis_end;
  };
  EvSlab sl{kl, vw, 0};
  sl.tw = tw;
  layout(sl);
  if (sl.bytes > 64 * 1024 &&
      hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)room) != hipSuccess) {
    (void)hipGetLastError();  // the default 64 KiB: the heap slab alone
    sl.vw = 0;
    sl.tw = 0;
    sl.kl = std::min(32, (64 * 1024) / (lanes * 24));
    layout(sl);
  }
  return sl;
}

}  // namespace cpr
