// wbx_mix_fam2.hip — mix_kernel instances of family 2: sessions whose clips are all 16-bit PCM at speeds up to 0.999 or
// exactly 1 (CD-rate files in a 48 kHz project): chunk modes U, I16, MU, WI, WIN, WINU; a chunk that holds a pre-rendered
// fp32 row next to 16-bit window rows goes one row at a time.
#include "wbx_mix.h"
#include "wbx_callback.h"

namespace wbx {

static const MixEntry kMixFam2[] = {
    WBX_MIX(2, true, 3, 2, 1, 1, 2, 64)
    WBX_MIX(4, true, 2, 2, 1, 1, 2, 128) WBX_MIX(1, true, 3, 2, 1, 1, 2, 128) WBX_MIX(2, true, 3, 2, 1, 1, 2, 128)
    WBX_MIX(2, true, 3, 2, 1, 1, 2, 256)
    WBX_MIX(2, true, 4, 2, 1, 1, 1, 256)
};

const char* launch_mix_fam2(const MixInstance& inst, const MixArgs& a, dim3 grid, hipStream_t s, hipEvent_t t0, hipEvent_t t1) {
  return launch_mix_from(kMixFam2, inst, a, grid, s, t0, t1);
}

static const CallbackEntry kCallbackFam2[] = {WBX_CALLBACK(2, 2)};

const char* launch_callback_fam2(const MixInstance& inst, const MixArgs& a, const PlanArgs& p, const SumArgs& s, const CallbackArgs& cb, hipStream_t st) {
  return launch_callback_from(kCallbackFam2, inst, a, p, s, cb, st);
}

}  // namespace wbx
