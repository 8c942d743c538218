// The replay of tests/step_schedule_check.cpp for the static schedules of six compute waves per streaming workgroup (-DZN_SK_CW=6:
// 2 parked tiles per wave, zn_api.hip's ZN_SK_T1 .. T3 of that build), and the cover of the fullest workgroup's share by both wave counts.
#define main zn_shipped_schedules_main
#include "step_schedule_check.cpp"
#undef main

// units of the fullest of nsw streaming workgroups at the Zonos-v0.1 shapes, against CW waves with T_* tiles each (stack_variant_ok's inequalities)
static void cover(const char* name, int nsw, int CW, int T_OUT, int T_FC1, int T_FC2, int T_IN, int P) {
  auto most = [&](int units) { return (units + nsw - 1) / nsw; };
  const int p_out = most(2048 / 2), p_fc1 = 2 * most(8192 / 2), p_qkv = most(3072 / 2), p_hd = most((9 * 1025 + 1) / 2);
  CHECK(p_out <= CW * T_OUT, "out_proj: %d row pairs > %d", p_out, CW * T_OUT);
  CHECK(4 * p_out <= CW * T_FC2, "fc2: %d quarter tiles > %d", 4 * p_out, CW * T_FC2);
  CHECK(p_fc1 <= CW * T_FC1, "fc1: %d rows > %d", p_fc1, CW * T_FC1);
  CHECK(p_qkv <= CW * T_IN && p_hd <= CW * T_IN, "in_proj / heads: %d / %d row pairs > %d", p_qkv, p_hd, CW * T_IN);
  CHECK(T_OUT <= P, "op 0's %d tiles are not all parked (%d)", T_OUT, P);
  CHECK(CW * P * 8192 + 26 * 1024 <= 160 * 1024, "LDS: %d KB of parked tiles", CW * P * 8);
  // a tighter schedule would not cover the share: the T_* are the smallest that do
  CHECK(p_out > CW * (T_OUT - 1) && 4 * p_out > CW * (T_FC2 - 1) && p_fc1 > CW * (T_FC1 - 1) && (p_qkv > CW * (T_IN - 1) || p_hd > CW * (T_IN - 1)), "a T_* is larger than needed");
  std::printf("%s: %d streaming workgroups, %d waves cover %d / %d / %d / %d units\n", name, nsw, CW, p_out, p_fc1, 4 * p_out, p_hd);
}

int main() {
  replay<1, 7, 4, 4, 3, 2, 0, 0xF, 0>("6 compute waves: step_kernel<4,1,7,4,4,6> (1 - 6 key blocks)");
  replay<1, 8, 4, 5, 3, 2, 0, 0xF, 0>("6 compute waves: step_kernel<4,1,8,4,5,8> (7 - 8 key blocks)");
  replay<2, 9, 5, 5, 3, 2, 0, 0xF, 0>("6 compute waves: step_kernel<4,2,9,5,5,12> (9 - 12 key blocks)");
  const char* name = "cover";
  cover(name, 256 - 48, 4, 2, 10, 5, 6, 4); cover(name, 256 - 64, 4, 2, 11, 6, 7, 4); cover(name, 256 - 96, 4, 2, 13, 7, 8, 4);
  cover(name, 256 - 48, 6, 1, 7, 4, 4, 2);  cover(name, 256 - 64, 6, 1, 8, 4, 5, 2);  cover(name, 256 - 96, 6, 2, 9, 5, 5, 2);
  return fails ? 1 : 0;
}
