// splice_plan_main.cpp — wbx_splice.h by itself (no HIP, no library): the tile tables of 40 generated part lists built into
// buffers of exactly their size and reduced to a checksum, the refusals walked.  tests/test_splice_host.py compiles this with
// -fsanitize=address,undefined and runs it directly; it generates the same lists and compares the checksums with a
// brute-force enumeration.
#include <cstdio>
#include <vector>

#include "../../whitebox_amd/csrc/wbx_splice.h"

static uint64_t state;
static uint64_t next() {   // the test's generator: a 64-bit LCG, the high 31 bits
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return state >> 33;
}

static wbx_splice_part part(uint32_t src, uint64_t first, uint64_t n, uint64_t at) {
  wbx_splice_part p{};
  p.src_clip = src;
  p.first_frame = first;
  p.n_frames = n;
  p.at = at;
  p.channel_mode = WBX_CH_KEEP;
  p.gain = 1.0f;
  return p;
}

int main() {
  const uint64_t kSrcFrames = 5000;
  const wbx_splice_source table[3] = {{0, 0, 0, 0, 0}, {1, 48000, kSrcFrames, WBX_FMT_F32, 0}, {1, 48000, 1u << 20, WBX_FMT_F32, 0}};
  const auto source_of = [&](uint32_t id) { return id < 3 ? &table[id] : nullptr; };
  for (uint32_t seed = 0; seed < 40; seed++) {
    state = seed;
    const uint64_t n_frames = 1 + next() % 5000;
    std::vector<wbx_splice_part> parts(1 + next() % 12);
    for (wbx_splice_part& p : parts) {
      const uint64_t n = 1 + next() % n_frames, at = next() % (n_frames - n + 1), first = next() % (kSrcFrames - n + 1);
      p = part(1, first, n, at);
    }
    wbx::SplicePlan plan;
    const char* why = "";
    if (wbx::splice_plan(1, n_frames, parts.data(), (uint32_t)parts.size(), source_of, &plan, &why) != WBX_OK) {
      std::printf("%u refused: %s\n", seed, why);
      return 1;
    }
    // once more into buffers of exactly the table's size: one word more written and the sanitizer says so
    std::vector<uint32_t> off((size_t)plan.n_tiles + 1), ent((size_t)plan.n_entries);
    wbx::splice_table(n_frames, parts.data(), (uint32_t)parts.size(), off.data(), ent.data());
    if (off != plan.tile_off || ent != plan.tile_parts || plan.rate != 48000) return 1;
    uint32_t sum = 0, i = 0;
    for (uint32_t v : off) sum ^= v * 2654435761u + i++;
    for (uint32_t v : ent) sum ^= v * 2654435761u + i++;
    std::printf("%u %08x\n", seed, sum);
  }

  wbx::SplicePlan plan;
  const char* why = "";
  const auto st = [&](uint32_t channels, uint64_t n_frames, const wbx_splice_part& p) {
    return wbx::splice_plan(channels, n_frames, &p, 1, source_of, &plan, &why);
  };
  const wbx_splice_part good = part(1, 0, 100, 0);
  wbx_splice_part p = good;
  bool ok = st(1, 100, good) == WBX_OK && plan.n_tiles == 1 && plan.n_entries == 1;
  ok = ok && wbx::splice_plan(1, 100, nullptr, 1, source_of, &plan, &why) == WBX_ERR_INVALID;
  ok = ok && wbx::splice_plan(1, 100, &good, 0, source_of, &plan, &why) == WBX_ERR_INVALID;
  ok = ok && st(1, 0, good) == WBX_ERR_INVALID && st(1, (1ull << 31) - 16, good) == WBX_ERR_INVALID;
  ok = ok && st(0, 100, good) == WBX_ERR_INVALID && st(3, 100, good) == WBX_ERR_INVALID && st(2, 100, good) == WBX_ERR_INVALID;
  ok = ok && st(1, 100, part(0, 0, 100, 0)) == WBX_ERR_INVALID && st(1, 100, part(7, 0, 100, 0)) == WBX_ERR_INVALID;
  ok = ok && st(1, 100, part(1, 0, 0, 0)) == WBX_ERR_INVALID && st(1, 100, part(1, 4950, 51, 0)) == WBX_ERR_INVALID;
  ok = ok && st(1, 100, part(1, ~0ull, 2, 0)) == WBX_ERR_INVALID && st(1, 100, part(1, 0, 100, 1)) == WBX_ERR_INVALID;
  ok = ok && st(1, 100, part(1, 0, 2, ~0ull)) == WBX_ERR_INVALID;
  p = good, p.flags = 2;
  ok = ok && st(1, 100, p) == WBX_ERR_INVALID;
  p = good, p.channel_mode = 6;
  ok = ok && st(1, 100, p) == WBX_ERR_INVALID;
  p = good, p.fade_in_shape = 3;
  ok = ok && st(1, 100, p) == WBX_ERR_INVALID;
  p = good, p.fade_out = 101;
  ok = ok && st(1, 100, p) == WBX_ERR_INVALID;
  p = good, p.channel_mode = WBX_CH_MONO_MIX;     // a stereo mode on a mono source
  ok = ok && st(1, 100, p) == WBX_ERR_INVALID;
  // the bounds: 65536 parts pass, one more does not; 65536 parts that touch 256 tiles each make 2^24 entries and pass, the
  // same parts one frame longer touch 257 and do not
  std::vector<wbx_splice_part> many(65536, part(1, 0, 1, 0));
  ok = ok && wbx::splice_plan(1, 100, many.data(), 65536, source_of, &plan, &why) == WBX_OK && plan.n_entries == 65536;
  many.push_back(good);
  ok = ok && wbx::splice_plan(1, 100, many.data(), 65537, source_of, &plan, &why) == WBX_ERR_UNSUPPORTED;
  many.assign(65536, part(2, 0, 256 * 512, 0));
  ok = ok && wbx::splice_plan(1, 1 << 18, many.data(), 65536, source_of, &plan, &why) == WBX_OK && plan.n_entries == (1u << 24) &&
       plan.tile_off[256] == (1u << 24) && plan.tile_off[512] == (1u << 24) && plan.tile_parts[(1u << 24) - 1] == 65535;
  many.assign(65536, part(2, 0, 256 * 512 + 1, 0));
  ok = ok && wbx::splice_plan(1, 1 << 18, many.data(), 65536, source_of, &plan, &why) == WBX_ERR_UNSUPPORTED;
  std::printf("refusals %s\n", ok ? "ok" : "WRONG");
  return ok ? 0 : 1;
}
