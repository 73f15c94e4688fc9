// Host check of alc_plan (csrc/predict_plan.h) against a table worked out by hand: exits non-zero at the first row that differs.
// bytes of a slot = 8 [NP MP_c + NP points + LD max(MP_c, points) + tiles_r MP_c], budget = half of the free bytes.
//   one chunk          E 3, m_c 300 (MP_c 384), m_r 300 (384, 3 tiles), NP 256, free 1e9: 8 (3 x 98304 + 1152) = 2 368 512 bytes, 211 slots fit -> 3, 384
//   padded last chunk  E 1, m_c 128, m_r 300, max_points 256 -> chunks of 256 and 44 points (the last padded to 128); 200 and 100 -> 128
//   group split        E 16, m_c 5000 (5120), m_r 10^4 (10112, 79 tiles), NP 2048, free 2e9: 8 x 52 308 992 = 418 471 936 bytes -> 2 of them in 1e9
//   refusal            the same at free 1e8: one 128-point chunk takes 8 x 21 638 144 = 173 105 152 bytes > 5e7
//   m_r = 10^6         E 1, m_c 128, NP 2048, free 3.4e10: all 1 000 064 points take 32.8e9 bytes; (2.125e9 - 1 262 208) / 4096 = 518 490 ->
//                      4050 tiles = 518 400 points, 16 997 028 864 bytes <= 1.7e10: two chunks, 518 400 + 481 600
//   chunk below MP_c   E 1, m_c 1000 (1024), m_r 2000 (2048, 16 tiles), NP 256, free 1.2e7: (750 000 - 278 528) / 512 = 920 < 1024, so
//                      (750 000 - 278 528 - 262 144) / 256 = 817 -> 768 points, 5 898 240 bytes (896 points: 6 160 384 > 6e6)
// tests/test_alc_host.py builds it with -fsanitize=address,undefined.
#include <cstdio>
#include <stdexcept>

#include "predict_plan.h"

struct Row {
  const char* name;
  long E, m_c, m_r;
  int NP;
  double free_b;
  int max_slots, max_points;
  bool refused;
  long slots, points, chunks, last;       // last: points of the last chunk
};

int main() {
  const Row table[] = {
      {"one chunk", 3, 300, 300, 256, 1e9, 0, 0, false, 3, 384, 1, 300},
      {"padded last chunk", 1, 128, 300, 256, 1e9, 0, 256, false, 1, 256, 2, 44},
      {"max_points rounds down", 1, 128, 300, 256, 1e9, 0, 200, false, 1, 128, 3, 44},
      {"max_points at least a tile", 1, 128, 300, 256, 1e9, 0, 100, false, 1, 128, 3, 44},
      {"max_points above the set", 1, 128, 300, 256, 1e9, 0, 100000, false, 1, 384, 1, 300},
      {"group split", 16, 5000, 10000, 2048, 2e9, 0, 0, false, 2, 10112, 1, 10000},
      {"group split, max_slots", 16, 5000, 10000, 2048, 2e9, 1, 0, false, 1, 10112, 1, 10000},
      {"max_slots above E", 3, 300, 300, 256, 1e9, 7, 0, false, 3, 384, 1, 300},
      {"refusal", 16, 5000, 10000, 2048, 1e8, 0, 0, true, 0, 0, 0, 0},
      {"a million reference points", 1, 128, 1000000, 2048, 3.4e10, 0, 0, false, 1, 518400, 2, 481600},
      {"chunk below MP_c", 1, 1000, 2000, 256, 1.2e7, 0, 0, false, 1, 768, 3, 464},
  };
  for (const Row& r : table) {
    mogp::AlcPlan p{0, 0};
    bool threw = false;
    try {
      p = mogp::alc_plan(r.E, r.m_c, r.m_r, r.NP, r.NP, r.free_b, r.max_slots, r.max_points);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (threw != r.refused) { std::printf("FAILED %s: refused %d, expected %d\n", r.name, (int)threw, (int)r.refused); return 1; }
    if (threw) continue;
    const long chunks = (r.m_r + p.points - 1) / p.points, last = r.m_r - (chunks - 1) * p.points;
    if (p.slots != r.slots || p.points != r.points || chunks != r.chunks || last != r.last) {
      std::printf("FAILED %s: slots %ld points %ld chunks %ld last %ld\n", r.name, p.slots, p.points, chunks, last);
      return 1;
    }
    const long tiles_r = mogp::alc_mp(r.m_r) / 128;
    if (p.points % 128 || p.points < 128 || (double)p.slots * mogp::alc_slot_bytes(r.NP, r.NP, mogp::alc_mp(r.m_c), p.points, tiles_r) > 0.5 * r.free_b) {
      std::printf("FAILED %s: the plan does not fit half of the free memory\n", r.name);
      return 1;
    }
  }
  // the byte counts the table was worked out from
  if (mogp::alc_slot_bytes(256, 256, 384, 384, 3) != 2368512.0 || mogp::alc_slot_bytes(2048, 2048, 5120, 10112, 79) != 418471936.0 ||
      mogp::alc_slot_bytes(2048, 2048, 5120, 128, 79) != 173105152.0 || mogp::alc_slot_bytes(2048, 2048, 128, 518400, 7813) != 16997028864.0 ||
      mogp::alc_slot_bytes(256, 256, 1024, 768, 16) != 5898240.0 || mogp::alc_slot_bytes(256, 256, 1024, 896, 16) != 6160384.0) {
    std::printf("FAILED the byte counts\n");
    return 1;
  }
  for (int bad = 0; bad < 2; ++bad) {
    bool threw = false;
    try {
      mogp::alc_plan(1, 10, 10, 256, 256, 1e9, bad == 0 ? -1 : 0, bad == 1 ? -1 : 0);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (!threw) { std::printf("FAILED negative max_* accepted\n"); return 1; }
  }
  // predict_cov's rule: V_1, V_2, the output and the K* scratch
  if (mogp::predict_cov_rule_bytes(300, 129, 256, 256) != 8.0 * (256.0 * (384 + 256) + 300.0 * 129 + 256.0 * 384)) {
    std::printf("FAILED predict_cov_rule_bytes\n");
    return 1;
  }
  std::printf("ok %d rows\n", (int)(sizeof(table) / sizeof(table[0])));
  return 0;
}
