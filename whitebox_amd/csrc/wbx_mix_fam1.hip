// wbx_mix_fam1.hip — mix_kernel instances of family 1, "everything": also per-frame taps (MODE_G: fp32 played faster than
// recorded, resampled integer PCM above 0.999), 16 / 24 / 32-bit window rows, windows of several storage formats in one
// chunk (MW, MWN).  Sessions with such clips take it; so does every block shape the lean families have no instance for.
#include "wbx_mix.h"
#include "wbx_callback.h"

namespace wbx {

static const MixEntry kMixFam1[] = {
    WBX_MIX_SHORT(1)
    WBX_MIX(2, false, 1, 1, 1, 1, 1, 256)   // any block shape: lane predicates, records read from LDS per lane
    WBX_MIX(2, true, 4, 1, 1, 1, 1, 256)
};

const char* launch_mix_fam1(const MixInstance& inst, const MixArgs& a, dim3 grid, hipStream_t s, hipEvent_t t0, hipEvent_t t1) {
  return launch_mix_from(kMixFam1, inst, a, grid, s, t0, t1);
}

static const CallbackEntry kCallbackFam1[] = {WBX_CALLBACK(2, 1)};

const char* launch_callback_fam1(const MixInstance& inst, const MixArgs& a, const PlanArgs& p, const SumArgs& s, const CallbackArgs& cb, hipStream_t st) {
  return launch_callback_from(kCallbackFam1, inst, a, p, s, cb, st);
}

}  // namespace wbx
