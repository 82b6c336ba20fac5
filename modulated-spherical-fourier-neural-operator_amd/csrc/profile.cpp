// Stage profiler of the block pipelines (msfno_profile_*).
#include "block.h"

namespace msfno {

// ---------------------------------------------------------------------------
// stage profiler (hipEvents on the caller's stream)
// ---------------------------------------------------------------------------
static const char* kStageNames[MSFNO_PROF_NSTAGES] = {
    "fft_fwd", "norm0_stats", "transpose_fwd", "legendre_fwd", "spectral_prep", "spectral_l0",
    "spectral_l1", "spectral_l2", "spectral_l3", "spectral_out", "linear_gather",
    "linear_contract", "linear_scatter", "legendre_inv", "transpose_inv", "fft_inv",
    "inner_skip", "norm1_film_fold", "mlp_fc1", "mlp_fc2", "out_affine", "band_pack",
    "band_exchange", "mlp_fused", "mlp_gen", "end"};

struct Profiler {
  bool on = false;
  struct Mark {
    int stage;
    hipStream_t stream;
    hipEvent_t ev;
  };
  std::vector<Mark> marks;
  std::vector<hipEvent_t> pool;
  // a stage lasts from its mark to the next mark recorded on the same stream
  void mark(int stage, hipStream_t s) {
    if (!on) return;
    hipEvent_t e;
    if (!pool.empty()) {
      e = pool.back();
      pool.pop_back();
    } else if (hipEventCreate(&e) != hipSuccess) {
      return;
    }
    if (hipEventRecord(e, s) != hipSuccess) {
      pool.push_back(e);
      return;
    }
    marks.push_back({stage, s, e});
  }
};
static Profiler g_prof;
void prof(int stage, hipStream_t s) { g_prof.mark(stage, s); }

}  // namespace msfno

using namespace msfno;

extern "C" {

int msfno_profile_mark(int stage, void* stream) {
  MSFNO_REQUIRE(stage >= 0 && stage <= ST_END, MSFNO_EINVAL, "profile stage out of range");
  prof(stage, (hipStream_t)stream);
  return MSFNO_OK;
}

int msfno_profile_enable(int on) {
  g_prof.on = on != 0;
  return MSFNO_OK;
}

const char* msfno_profile_stage_name(int stage) {
  if (stage < 0 || stage >= MSFNO_PROF_NSTAGES || !kStageNames[stage]) return "";
  return kStageNames[stage];
}

int msfno_profile_collect(double* total_ms, int* counts) {
  auto& mk = g_prof.marks;
  for (auto& m : mk) MSFNO_CHECK_HIP(hipEventSynchronize(m.ev));
  for (size_t i = 0; i < mk.size(); ++i) {
    if (mk[i].stage == ST_END) continue;
    size_t j = i + 1;
    while (j < mk.size() && mk[j].stream != mk[i].stream) ++j;
    if (j == mk.size()) continue;
    float ms = 0.f;
    MSFNO_CHECK_HIP(hipEventElapsedTime(&ms, mk[i].ev, mk[j].ev));
    if (total_ms) total_ms[mk[i].stage] += ms;
    if (counts) counts[mk[i].stage] += 1;
  }
  for (auto& m : mk) g_prof.pool.push_back(m.ev);
  mk.clear();
  return MSFNO_OK;
}

}  // extern "C"
