// dynamics_main.cpp — wbx_dynamics.h alone, stand-alone (its own main, g++ only, no device, no library): what
// tests/test_dynamics_host.py runs under AddressSanitizer and UBSan.  Reads a text file of cases, one per line:
//   t <kind> <T> <ratio> <knee> <range> <cap>   -> "t <status> <fnv-1a of the cap doubles' bits> <first> <last>"; an accepted
//                                                  design of cap == 3073 becomes the CURRENT table
//   m <entry> <bits>                            -> (nothing) the current table's entry is overwritten
//   k <sense>                                   -> "k <status of dynamics_table_check> <lo>" for the current table
//   l <level bits>                              -> "l <dynamics_lookup of the current table>"
//   c <n> <sense> <drive> <key_gain> <makeup> <A> <H> <R> <keyed> <table: 1, or 0 for NULL>
//                                               -> "c <status of dynamics_check_args>"
// doubles travel as the 16 hex digits of their bits.  The design's buffer holds exactly <cap> doubles (a design that wrote
// past 3073, or into a capacity it should have refused, is the sanitizer's to see) and starts as 7.0.  Ends with
// "dynamics ok".
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../whitebox_amd/csrc/wbx_dynamics.h"

static double from_bits(const std::string& w) { return wbx::dyn_from_bits(std::stoull(w, nullptr, 16)); }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  std::vector<double> current(wbx::kDynTable, 1.0);
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string tag;
    ss >> tag;
    if (tag == "t") {
      int kind;
      std::string T, ratio, knee, range;
      size_t cap;
      ss >> kind >> T >> ratio >> knee >> range >> cap;
      std::vector<double> out(cap, 7.0);
      const wbx_status st = wbx::dynamics_table(kind, from_bits(T), from_bits(ratio), from_bits(knee), from_bits(range), out.data(), cap);
      uint64_t h = 1469598103934665603ull;
      for (double v : out) {
        const uint64_t u = wbx::dyn_bits(v);
        for (int i = 0; i < 8; i++) h = (h ^ ((u >> (8 * i)) & 0xFFu)) * 1099511628211ull;
      }
      std::printf("t %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", (int)st, h, cap ? wbx::dyn_bits(out.front()) : 0,
                  cap ? wbx::dyn_bits(out.back()) : 0);
      if (st == WBX_OK && cap == wbx::kDynTable) current = out;
    } else if (tag == "m") {
      uint32_t entry;
      std::string bits;
      ss >> entry >> bits;
      if (entry >= wbx::kDynTable) return 3;
      current[entry] = from_bits(bits);
    } else if (tag == "k") {
      int sense;
      ss >> sense;
      double lo = 7.0;
      const wbx_status st = wbx::dynamics_table_check(current.data(), sense, &lo);
      std::printf("k %d %016" PRIx64 "\n", (int)st, wbx::dyn_bits(lo));
    } else if (tag == "l") {
      std::string level;
      ss >> level;
      std::printf("l %016" PRIx64 "\n", wbx::dyn_bits(wbx::dynamics_lookup(current.data(), from_bits(level))));
    } else if (tag == "c") {
      wbx::DynCall k{};
      std::string drive, key_gain, makeup;
      int keyed, has_table;
      ss >> k.n_frames >> k.sense >> drive >> key_gain >> makeup >> k.lookahead >> k.hold >> k.release >> keyed >> has_table;
      k.drive = from_bits(drive), k.key_gain = from_bits(key_gain), k.makeup = from_bits(makeup);
      k.keyed = keyed != 0;
      k.table = has_table ? current.data() : nullptr;
      const char* why = "";
      double lo = 7.0;
      const wbx_status st = wbx::dynamics_check_args(k, &lo, &why);
      if ((st == WBX_OK) != (why[0] == 0)) return 4;           // a refusal says why, an acceptance nothing
      std::printf("c %d\n", (int)st);
    }
  }
  double small[4];
  if (wbx::dynamics_table(WBX_DYN_COMPRESS, -18.0, 4.0, 6.0, -40.0, nullptr, wbx::kDynTable) != WBX_ERR_INVALID) return 5;
  if (wbx::dynamics_table(WBX_DYN_COMPRESS, -18.0, 4.0, 6.0, -40.0, small, 4) != WBX_ERR_INVALID) return 6;
  if (wbx::dynamics_table_check(nullptr, WBX_DYN_GATE, nullptr) != WBX_ERR_INVALID) return 7;
  if (wbx::dyn_exp2(0.0) != 1.0 || wbx::dyn_exp2(-0.0) != 1.0 || wbx::dyn_exp2(-1.0) != 0.5 || wbx::dyn_log2_mantissa(1.0) != 0.0) return 8;
  static_assert(wbx::kDynTable == 3073 && wbx::kDynCells == 64 && wbx::kDynMinExp == -40, "the header's text names these");
  std::printf("dynamics ok\n");
  return 0;
}
