// wbx_mix_fam3.hip — mix_kernel instances of family 3: family 1's chunk modes without the per-frame taps (MODE_G).  Sessions
// with resampled integer PCM (24-bit stems at another rate, 16-bit loops next to them) but no clip played faster than
// recorded take it: without that mode the instance with both channels of a frame per lane fits its register budget.
#include "wbx_mix.h"

namespace wbx {

static const MixEntry kMixFam3[] = {WBX_MIX(2, true, 3, 3, 1, 1, 2, 128) WBX_MIX(1, true, 3, 3, 1, 1, 2, 128)};

const char* launch_mix_fam3(const MixInstance& inst, const MixArgs& a, dim3 grid, hipStream_t s, hipEvent_t t0, hipEvent_t t1) {
  return launch_mix_from(kMixFam3, inst, a, grid, s, t0, t1);
}

}  // namespace wbx
