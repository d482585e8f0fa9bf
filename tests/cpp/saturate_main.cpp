// saturate_main.cpp — wbx_saturate.h alone, stand-alone (its own main, g++ only, no device, no library): what
// tests/test_saturate_host.py runs under AddressSanitizer and UBSan.  Reads a text file of cases, one per line (doubles and
// table entries as the hex of their bits):
//   t <kind> <bias bits>                       -> "t <status> <fnv-1a 64 of the table's bytes>"; the table stays current
//   r <seed>                                   -> "r": the current table becomes a hand-drawn one (an LCG, entries in +-2)
//   p <index> <entry bits>                     -> "p": one entry of the current table is replaced
//   k                                          -> "k <status of saturate_table_check on the current table>"
//   l <d bits>                                 -> "l <bits of saturate_lookup(current table, d)>"
//   c <n> <os> <quality> <table: 0 NULL, 1 current> <drive bits> <makeup bits> -> "c <status of saturate_check_args>"
//   s <os> <quality> <channels> <n>            -> "s <tile> <mid_span> <src_span> <lds_bytes> <n_tiles>"
// Ends with "saturate ok".
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../whitebox_amd/csrc/wbx_saturate.h"

static double from_hex(const std::string& s) { return wbx::dyn_from_bits(std::stoull(s, nullptr, 16)); }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  std::vector<double> tab(wbx::kSatTable, 0.0);                  // exactly the table's length: ASan sees one entry too many
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string tag;
    ss >> tag;
    if (tag == "t") {
      int kind;
      std::string bias;
      ss >> kind >> bias;
      const wbx_status st = wbx::saturate_table(kind, from_hex(bias), tab.data(), tab.size());
      if (wbx::saturate_table(kind, from_hex(bias), tab.data(), tab.size() - 1u) != WBX_ERR_INVALID) return 3;
      uint64_t h = 1469598103934665603ull;
      for (double v : tab) {
        const uint64_t u = wbx::dyn_bits(v);
        for (int b = 0; b < 8; b++) h = (h ^ ((u >> (8 * b)) & 0xFFu)) * 1099511628211ull;
      }
      std::printf("t %d %016" PRIx64 "\n", (int)st, h);
    } else if (tag == "r") {
      uint64_t x;
      ss >> x;
      for (double& v : tab) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        v = (double)(int64_t)(x >> 11) * 0x1p-51 - 2.0;            // 53 bits in [0, 4), less 2
      }
      std::printf("r\n");
    } else if (tag == "p") {
      uint32_t at;
      std::string v;
      ss >> at >> v;
      if (at >= wbx::kSatTable) return 4;
      tab[at] = from_hex(v);
      std::printf("p\n");
    } else if (tag == "k") {
      std::printf("k %d\n", (int)wbx::saturate_table_check(tab.data()));
    } else if (tag == "l") {
      std::string d;
      ss >> d;
      std::printf("l %016" PRIx64 "\n", wbx::dyn_bits(wbx::saturate_lookup(tab.data(), from_hex(d))));
    } else if (tag == "c") {
      wbx::SatCall k{};
      int has_table;
      std::string drive, makeup;
      ss >> k.n_frames >> k.os >> k.quality >> has_table >> drive >> makeup;
      k.table = has_table ? tab.data() : nullptr;
      k.drive = from_hex(drive), k.makeup = from_hex(makeup);
      const char* why = "";
      const wbx_status st = wbx::saturate_check_args(k, &why);
      if ((st == WBX_OK) != (why[0] == 0)) return 5;             // a refusal says why, an acceptance nothing
      std::printf("c %d\n", (int)st);
    } else if (tag == "s") {
      uint32_t os, channels;
      int quality;
      uint64_t n;
      ss >> os >> quality >> channels >> n;
      const wbx::SatShape s = wbx::saturate_shape(os, quality, channels, n);
      // what the kernel relies on: a lane owns 4 frames of the tile, the tiles cover the range, the LDS needs no opt-in and
      // holds the fold's 256 records of 24 bytes
      if (s.tile % 256u || s.tile < 256u || s.tile > 1024u || (uint64_t)s.n_tiles * s.tile < n || s.n_tiles > 1u << 21) return 6;
      if (os > 1u && (s.lds_bytes > 65536u || s.lds_bytes < 6144u || s.lds_bytes != channels * 4u * (s.plane * os + s.row))) return 7;
      if (os > 1u && (s.plane != s.tile + 2u * s.Z || s.row != s.tile + 4u * s.Z || s.plane % 4u || s.row % 4u)) return 8;
      std::printf("s %u %u %u %u %u\n", (unsigned)s.tile, (unsigned)s.mid_span, (unsigned)s.src_span, (unsigned)s.lds_bytes, (unsigned)s.n_tiles);
    }
  }
  static_assert(wbx::kSatTable == 16385 && sizeof(wbx_saturate_stats) == 24, "the header's text names these");
  std::printf("saturate ok\n");
  return 0;
}
