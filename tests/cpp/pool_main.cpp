// pool_main.cpp — wbx_pool.h by itself (no HIP, no library, no Python): the scripts named on the command line, written by
// tests/test_pool_model.py, run through pool_sim.cpp's interface with the slabs' books checked here after every line.
// The test compiles this with -fsanitize=address,undefined -D_GLIBCXX_DEBUG and runs it directly.
//   T key need own_bytes where slab off    a take and where tests/pool_model.py places it
//   G key                                  a give
//   L bytes                                wbx_clip_pool_limit
//   F 0|1                                  the driver is out of memory
// Prints "<script> <takes> <digest of the placements>" per script; the first wrong line ends the run with status 1.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "pool_sim.cpp"

namespace {

struct Live {
  uint32_t id;
  int slab;
  uint64_t off, len;
};

bool books_ok(void* h, const std::map<long, Live>& live, std::string* why) {
  uint32_t n = 0;
  uint64_t reserved = 0, bytes_live = 0, calls = 0, sum = 0, info[4];
  psim_stats(h, &n, &reserved, &bytes_live, &calls);
  for (auto& kv : live) sum += kv.second.len;
  if (sum != bytes_live) return *why = "bytes_live", false;
  for (uint32_t si = 0; si < n; si++) {
    const int nh = psim_dump(h, si, info, nullptr, 0);
    std::vector<uint64_t> holes(2 * (size_t)std::max(nh, 1));
    psim_dump(h, si, info, holes.data(), (uint32_t)nh);
    std::vector<std::pair<uint64_t, uint64_t>> pieces;
    for (int k = 0; k < nh; k++) {
      if (!holes[2 * k + 1]) return *why = "an empty hole", false;
      if (k && holes[2 * k - 2] + holes[2 * k - 1] >= holes[2 * k]) return *why = "holes unsorted, overlapping or adjacent", false;
      pieces.emplace_back(holes[2 * k], holes[2 * k + 1]);
    }
    if (nh && holes[2 * nh - 2] + holes[2 * nh - 1] >= info[1]) return *why = "a hole reaches the bump pointer", false;
    uint64_t n_live = 0, live_bytes = 0;
    for (auto& kv : live)
      if (kv.second.slab == (int)si) {
        pieces.emplace_back(kv.second.off, kv.second.len);
        n_live++;
        live_bytes += kv.second.len;
      }
    std::sort(pieces.begin(), pieces.end());
    uint64_t pos = 0;
    for (auto& p : pieces) {
      if (p.first != pos) return *why = "holes and live extents do not tile [0, used)", false;
      pos += p.second;
    }
    if (pos != info[1] || info[1] > info[0]) return *why = "used", false;
    if (n_live != info[2] || live_bytes != info[3]) return *why = "live count or bytes", false;
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  for (int a = 1; a < argc; a++) {
    std::FILE* f = std::fopen(argv[a], "r");
    if (!f) return std::printf("cannot read %s\n", argv[a]), 1;
    void* h = psim_create();
    std::map<long, Live> live;
    uint64_t digest = 0xCBF29CE484222325ull, takes = 0;
    char line[256];
    int lineno = 0;
    std::string why;
    while (std::fgets(line, sizeof line, f)) {
      lineno++;
      long key = 0, want_where = 0, want_slab = 0;
      unsigned long long need = 0, own = 0, want_off = 0, v = 0;
      if (std::sscanf(line, "T %ld %llu %llu %ld %ld %llu", &key, &need, &own, &want_where, &want_slab, &want_off) == 6) {
        Live e{};
        int32_t slab = 0;
        uint64_t off = 0;
        const int where = psim_take(h, need, own, 1, &e.id, &slab, &off);
        if (where != want_where || slab != want_slab || off != want_off)
          return std::printf("%s:%d: placed %d/%d/%" PRIu64 ", the model %ld/%ld/%llu\n", argv[a], lineno, where, (int)slab, off, want_where,
                             want_slab, want_off), 1;
        for (uint64_t x : {(uint64_t)where, (uint64_t)(slab + 1), off}) digest = (digest ^ x) * 0x100000001B3ull;
        takes++;
        if (where == wbx::POOL_IN_SLAB || where == wbx::POOL_OWN) {
          e.slab = slab;
          e.off = off;
          e.len = where == wbx::POOL_IN_SLAB ? need : own;
          live[key] = e;
        }
      } else if (std::sscanf(line, "G %ld", &key) == 1) {
        auto it = live.find(key);
        if (it == live.end() || psim_give(h, it->second.id) != 0) return std::printf("%s:%d: nothing to give\n", argv[a], lineno), 1;
        live.erase(it);
      } else if (std::sscanf(line, "L %llu", &v) == 1) {
        psim_set_limit(h, v);
      } else if (std::sscanf(line, "F %llu", &v) == 1) {
        psim_set_driver_fails(h, (int)v);
      } else {
        return std::printf("%s:%d: not a script line\n", argv[a], lineno), 1;
      }
      if (!books_ok(h, live, &why)) return std::printf("%s:%d: %s\n", argv[a], lineno, why.c_str()), 1;
    }
    std::fclose(f);
    uint32_t n = 0;
    uint64_t reserved = 0, bytes_live = 0, calls = 0, info[4];
    psim_stats(h, &n, &reserved, &bytes_live, &calls);
    bool empty = live.empty() && bytes_live == 0;
    for (uint32_t si = 0; si < n; si++) empty = empty && psim_dump(h, si, info, nullptr, 0) == 0 && info[1] == 0 && info[2] == 0;
    if (!empty) return std::printf("%s: the pool is not empty at the end\n", argv[a]), 1;
    psim_destroy(h);
    std::string name = argv[a];
    name = name.substr(name.find_last_of('/') + 1);
    name = name.substr(0, name.rfind('.'));
    std::printf("%s %" PRIu64 " %016" PRIx64 "\n", name.c_str(), takes, digest);
  }
  return 0;
}
