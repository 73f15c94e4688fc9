// Host check of alc_batch_plan (csrc/predict_plan.h) against a table worked out by hand: exits non-zero at the first row that differs.
// bytes of a slot, ext = roundup(steps, 16), MPx = max(MP_c, MP_r), tiles_r = MP_r / 128, budget = half of the free bytes:
//   8 [(NP + ext) MP_c + (NP + ext) MP_r + LD MPx + tiles_r MP_c]  +  8 NP MPx  +  8 (NP / 128 + 2) MPx  +  8 (2 MP_c + MP_r + 2 ext)  +  4 (2 MP_c + ext)
//   one group      E 3, m_c 300 (384), m_r 300 (384, 3 tiles), 17 steps (ext 32), NP 256, free 1e9:
//                  8 (288 x 384 + 288 x 384 + 256 x 384 + 3 x 384) = 8 x 320 640 = 2 565 120;  + 786 432 + 8 x 4 x 384 = 12 288
//                  + 8 (768 + 384 + 64) = 9 728 + 4 (768 + 32) = 3 200  ->  3 376 768 bytes, 148 fit 5e8 -> 3 slots
//   group split    E 16, m_c 5000 (5120), m_r 10^4 (10112, 79 tiles), 16 steps (ext 16), NP 2048, free 4e9:
//                  8 (2064 x 5120 + 2064 x 10112 + 2048 x 10112 + 79 x 5120) = 8 x 52 552 704 = 420 421 632;  + 8 x 2048 x 10112 = 165 675 008
//                  + 8 x 18 x 10112 = 1 456 128 + 8 (10240 + 10112 + 32) = 163 072 + 4 (10240 + 16) = 41 024  ->  587 756 864 bytes,
//                  3 of them in 2e9 -> groups of 3; max_slots 2 -> 2; max_slots 1 -> 1
//   total refusal  the same with total: 16 emulators need 9 404 109 824 bytes > 2e9; with E 3 the three fit one group (max_slots ignored)
//   one emulator   the same at free 1e9: 587 756 864 > 5e8, refused in either mode
// tests/test_alc_batch_host.py builds it with -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "predict_plan.h"

struct Row {
  const char* name;
  long E, m_c, m_r, steps;
  int NP;
  double free_b;
  int max_slots;
  bool total, refused;
  long slots;
  const char* says;       // what the refusal must name (null: nothing asked)
};

int main() {
  const Row table[] = {
      {"one group", 3, 300, 300, 17, 256, 1e9, 0, false, false, 3, nullptr},
      {"one group, total", 3, 300, 300, 17, 256, 1e9, 0, true, false, 3, nullptr},
      {"max_slots", 3, 300, 300, 17, 256, 1e9, 1, false, false, 1, nullptr},
      {"max_slots above E", 3, 300, 300, 17, 256, 1e9, 7, false, false, 3, nullptr},
      {"group split", 16, 5000, 10000, 16, 2048, 4e9, 0, false, false, 3, nullptr},
      {"group split, max_slots 2", 16, 5000, 10000, 16, 2048, 4e9, 2, false, false, 2, nullptr},
      {"group split, max_slots 1", 16, 5000, 10000, 16, 2048, 4e9, 1, false, false, 1, nullptr},
      {"total refusal", 16, 5000, 10000, 16, 2048, 4e9, 0, true, true, 0, "9404109824"},
      {"total, three fit", 3, 5000, 10000, 16, 2048, 4e9, 1, true, false, 3, nullptr},
      {"one emulator", 16, 5000, 10000, 16, 2048, 1e9, 0, false, true, 0, "587756864"},
      {"one emulator, total", 1, 5000, 10000, 16, 2048, 1e9, 0, true, true, 0, "587756864"},
  };
  for (const Row& r : table) {
    long slots = 0;
    bool threw = false;
    std::string msg;
    try {
      slots = mogp::alc_batch_plan(r.E, r.m_c, r.m_r, r.steps, r.NP, r.NP, r.free_b, r.max_slots, r.total);
    } catch (const std::runtime_error& e) {
      threw = true;
      msg = e.what();
    }
    if (threw != r.refused) { std::printf("FAILED %s: refused %d, expected %d\n", r.name, (int)threw, (int)r.refused); return 1; }
    if (threw) {
      if (r.says && msg.find(r.says) == std::string::npos) { std::printf("FAILED %s: the refusal does not name %s: %s\n", r.name, r.says, msg.c_str()); return 1; }
      continue;
    }
    if (slots != r.slots) { std::printf("FAILED %s: slots %ld\n", r.name, slots); return 1; }
    const long MPc = mogp::alc_mp(r.m_c), MPr = mogp::alc_mp(r.m_r);
    if ((double)slots * mogp::alc_batch_slot_bytes(r.NP, r.NP, MPc, MPr, MPr / 128, mogp::alc_ext_rows(r.steps)) > 0.5 * r.free_b) {
      std::printf("FAILED %s: the plan does not fit half of the free memory\n", r.name);
      return 1;
    }
  }
  // the byte counts and the extension rows the table was worked out from
  if (mogp::alc_batch_slot_bytes(256, 256, 384, 384, 3, 32) != 3376768.0 || mogp::alc_batch_slot_bytes(2048, 2048, 5120, 10112, 79, 16) != 587756864.0 ||
      mogp::alc_slot_bytes(2064, 2048, 5120, 10112, 79) != 420421632.0) {
    std::printf("FAILED the byte counts\n");
    return 1;
  }
  if (mogp::alc_ext_rows(1) != 16 || mogp::alc_ext_rows(16) != 16 || mogp::alc_ext_rows(17) != 32 || mogp::alc_ext_rows(0) != 16) {
    std::printf("FAILED alc_ext_rows\n");
    return 1;
  }
  bool threw = false;
  try {
    mogp::alc_batch_plan(1, 10, 10, 3, 256, 256, 1e9, -1, false);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  if (!threw) { std::printf("FAILED negative max_slots accepted\n"); return 1; }
  std::printf("ok %d rows\n", (int)(sizeof(table) / sizeof(table[0])));
  return 0;
}
