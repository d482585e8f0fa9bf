// wbx_mix_fam0.hip — mix_kernel instances of family 0: fp32 rows (unity / 5-sample window) and integer PCM at unity speed
// (chunk modes U, W, WN, WNU, I16, I32, MU, MIXED).  What the BASELINE configurations 2-5 take.
#include "wbx_mix.h"
#include "wbx_callback.h"

namespace wbx {

static const MixEntry kMixFam0[] = {
    // both channels of a frame in one lane: 256-frame stereo blocks (one wave = one block) ...
    WBX_MIX(2, true, 3, 0, 1, 1, 2, 64)
    WBX_MIX_SHORT(0)
    // ... 512-frame ones, 1024-frame ones
    WBX_MIX(1, true, 3, 0, 1, 1, 2, 128) WBX_MIX(4, true, 2, 0, 1, 1, 2, 128) WBX_MIX(2, true, 3, 0, 1, 1, 2, 128)
    WBX_MIX(2, true, 3, 0, 1, 1, 2, 256)
    WBX_MIX(2, true, 4, 0, 1, 1, 1, 256) WBX_MIX(4, true, 3, 0, 1, 1, 1, 256) WBX_MIX(8, true, 2, 0, 1, 1, 1, 256)
};

const char* launch_mix_fam0(const MixInstance& inst, const MixArgs& a, dim3 grid, hipStream_t s, hipEvent_t t0, hipEvent_t t1) {
  return launch_mix_from(kMixFam0, inst, a, grid, s, t0, t1);
}

// the one-launch callback (wbx_callback.h)
static const CallbackEntry kCallbackFam0[] = {WBX_CALLBACK(8, 0) WBX_CALLBACK(4, 0) WBX_CALLBACK(2, 0)};

const char* launch_callback_fam0(const MixInstance& inst, const MixArgs& a, const PlanArgs& p, const SumArgs& s, const CallbackArgs& cb, hipStream_t st) {
  return launch_callback_from(kCallbackFam0, inst, a, p, s, cb, st);
}

}  // namespace wbx
