// csrc/mcs_options.h on its own, in a program with its own main (built with -fsanitize=address,undefined by tests/test_options.py):
// the option table, the three rules by which a variable seeds a default, the precedence default < environment < caller's list,
// use_env = 0, and every refusal of the check.  Includes nothing else of the project; no GPU, no HIP.
#include "mcs_options.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static void put(const char* name, const char* v) { if (v) setenv(name, v, 1); else unsetenv(name); }
static void clear_env() { for (const McsOptionRow& r : kMcsOptions) unsetenv(r.env); }
static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }
static int64_t from_env(int key, const char* v) { put(kMcsOptions[key].env, v); return mcs_option_from_env(kMcsOptions[key]); }

static void test_table() {
  CHECK(MCS_OPT_COUNT == 14);
  for (int k = 0; k < MCS_OPT_COUNT; ++k) {
    const McsOptionRow* r = mcs_option_row(k);
    CHECK(r && r->key == k && r->min <= r->dflt && r->dflt <= r->max && std::strncmp(r->env, "MCS_", 4) == 0);
    for (int j = 0; j < k; ++j) CHECK(std::strcmp(kMcsOptions[j].name, r->name) != 0 && std::strcmp(kMcsOptions[j].env, r->env) != 0);
    CHECK(has(mcs_option_label(*r), r->name) && has(mcs_option_label(*r), "MCS_OPT_"));
  }
  CHECK(!mcs_option_row(-1) && !mcs_option_row(MCS_OPT_COUNT));
  CHECK(mcs_option_label(kMcsOptions[MCS_OPT_DEFER_K]) == "option defer_k (MCS_OPT_DEFER_K)");
}

// the rules, as the library has always read these variables
static void test_env_rules() {
  clear_env();
  // env_on: the first character '1'
  CHECK(from_env(MCS_OPT_FORCE_GENERAL, nullptr) == 0);
  CHECK(from_env(MCS_OPT_FORCE_GENERAL, "1") == 1);
  CHECK(from_env(MCS_OPT_FORCE_GENERAL, "1x") == 1);
  CHECK(from_env(MCS_OPT_FORCE_GENERAL, "0") == 0);
  CHECK(from_env(MCS_OPT_FORCE_GENERAL, "") == 0);
  CHECK(from_env(MCS_OPT_FORCE_GENERAL, "yes") == 0);
  CHECK(from_env(MCS_OPT_FORCE_GENERAL, "01") == 0);
  CHECK(from_env(MCS_OPT_F32_LOOP, "1x") == 1 && from_env(MCS_OPT_F32_EXACT, "11") == 1);
  // ... inverted
  CHECK(from_env(MCS_OPT_TALLY_REPLICAS, nullptr) == 1);
  CHECK(from_env(MCS_OPT_TALLY_REPLICAS, "1") == 0);
  CHECK(from_env(MCS_OPT_TALLY_REPLICAS, "1x") == 0);
  CHECK(from_env(MCS_OPT_TALLY_REPLICAS, "0") == 1);
  CHECK(from_env(MCS_OPT_TALLY_REPLICAS, "on") == 1);
  // env_not_off: off iff the first character is '0'
  for (int key : {MCS_OPT_TAIL_MERGE, MCS_OPT_PARK, MCS_OPT_TAIL_RING}) {
    CHECK(from_env(key, nullptr) == 1);
    CHECK(from_env(key, "0") == 0);
    CHECK(from_env(key, "01") == 0);
    CHECK(from_env(key, "1") == 1);
    CHECK(from_env(key, "") == 1);
    CHECK(from_env(key, "off") == 1);
  }
  // tri-state
  CHECK(from_env(MCS_OPT_K1_WS, nullptr) == 2);
  CHECK(from_env(MCS_OPT_K1_WS, "0") == 0);
  CHECK(from_env(MCS_OPT_K1_WS, "1") == 1);
  CHECK(from_env(MCS_OPT_K1_WS, "10") == 1);
  CHECK(from_env(MCS_OPT_K1_WS, "7") == 2);
  CHECK(from_env(MCS_OPT_K1_WS, "2") == 2);
  CHECK(from_env(MCS_OPT_K1_WS, "") == 2);
  // integers: inside the range, else the default
  for (const McsOptionRow& r : kMcsOptions) {
    if (r.rule != MCS_ENV_INT) continue;
    CHECK(from_env(r.key, nullptr) == r.dflt);
    CHECK(from_env(r.key, std::to_string(r.min).c_str()) == r.min);
    CHECK(from_env(r.key, std::to_string(r.max).c_str()) == r.max);
    CHECK(from_env(r.key, std::to_string(r.min - 1).c_str()) == r.dflt);
    if (r.max < INT64_MAX) CHECK(from_env(r.key, std::to_string(r.max + 1).c_str()) == r.dflt);
    CHECK(from_env(r.key, "abc") == (r.min <= 0 ? 0 : r.dflt));      // (atoll gives 0, which REFILL_MIN and DEFER_K do not allow)
    CHECK(from_env(r.key, "") == (r.min <= 0 ? 0 : r.dflt));
    put(r.env, nullptr);
  }
  CHECK(from_env(MCS_OPT_DEFER_K, "99") == 8 && from_env(MCS_OPT_DEFER_K, "1") == 1 && from_env(MCS_OPT_DEFER_K, "x") == 8);
  CHECK(from_env(MCS_OPT_REFILL_MIN, "20") == 20 && from_env(MCS_OPT_REFILL_MIN, "0") == 12 && from_env(MCS_OPT_REFILL_MIN, "49") == 12);
  CHECK(from_env(MCS_OPT_TAIL_LOOP, "33") == 12 && from_env(MCS_OPT_TAIL_LOOP, "0") == 0 && from_env(MCS_OPT_TAIL_LOOP, "7up") == 7);
  CHECK(from_env(MCS_OPT_WS_AUTO_MIN, "-1") == 6000000 && from_env(MCS_OPT_WS_AUTO_MIN, "0") == 0);
  CHECK(from_env(MCS_OPT_PIPE_SIDE_CUS, "129") == 12 && from_env(MCS_OPT_PIPE_SIDE_CUS, "128") == 128);
  CHECK(from_env(MCS_OPT_TAIL_BUDGET, "16777217") == 0 && from_env(MCS_OPT_TAIL_BUDGET, "16777216") == 16777216);
  // the functions themselves, by name
  put("MCS_X_TEST", "1x"); CHECK(env_on("MCS_X_TEST") && env_not_off("MCS_X_TEST") && env_tristate("MCS_X_TEST") == 1);
  put("MCS_X_TEST", nullptr); CHECK(!env_on("MCS_X_TEST") && env_not_off("MCS_X_TEST") && env_tristate("MCS_X_TEST") == 2);
  CHECK(env_int("MCS_X_TEST", 1, 5, 3) == 3);
  put("MCS_X_TEST", "5"); CHECK(env_int("MCS_X_TEST", 1, 5, 3) == 5);
  put("MCS_X_TEST", "6"); CHECK(env_int("MCS_X_TEST", 1, 5, 3) == 3);
  put("MCS_X_TEST", nullptr);
  clear_env();
}

static void test_precedence() {
  int64_t v[MCS_OPT_COUNT];
  std::string msg;
  clear_env();
  // nothing given: the built-in defaults, with and without the environment
  for (int use_env = 0; use_env < 2; ++use_env) {
    CHECK(mcs_options_resolve(nullptr, nullptr, 0, use_env != 0, 0, v, &msg) == MCS_OPTION_OK);
    for (int k = 0; k < MCS_OPT_COUNT; ++k) CHECK(v[k] == kMcsOptions[k].dflt);
  }
  const int64_t want_dflt[MCS_OPT_COUNT] = {0, 2, 6000000, 1, 1, 1, 12, 12, 8, 0, 12, 1, 0, 0};
  for (int k = 0; k < MCS_OPT_COUNT; ++k) CHECK(v[k] == want_dflt[k]);
  // default < environment
  put("MCS_FORCE_GENERAL", "1"); put("MCS_DEFER_K", "3"); put("MCS_K1_WS", "0"); put("MCS_TALLY_REPLICAS_OFF", "1"); put("MCS_PARK", "0");
  put("MCS_REFILL_MIN", "77");      // (outside: the default stays, silently)
  put("MCS_F32_EXACT", "1");        // (does not apply to a fp64 context: carried, as ever)
  CHECK(mcs_options_resolve(nullptr, nullptr, 0, true, 0, v, &msg) == MCS_OPTION_OK);
  CHECK(v[MCS_OPT_FORCE_GENERAL] == 1 && v[MCS_OPT_DEFER_K] == 3 && v[MCS_OPT_K1_WS] == 0 && v[MCS_OPT_TALLY_REPLICAS] == 0 && v[MCS_OPT_PARK] == 0);
  CHECK(v[MCS_OPT_REFILL_MIN] == 12 && v[MCS_OPT_F32_EXACT] == 1 && v[MCS_OPT_TAIL_LOOP] == 12);
  // environment < caller; the last of a key given twice
  const int32_t keys[] = {MCS_OPT_FORCE_GENERAL, MCS_OPT_K1_WS, MCS_OPT_TAIL_LOOP, MCS_OPT_TAIL_LOOP};
  const int64_t vals[] = {0, 1, 5, 6};
  CHECK(mcs_options_resolve(keys, vals, 4, true, 0, v, &msg) == MCS_OPTION_OK);
  CHECK(v[MCS_OPT_FORCE_GENERAL] == 0 && v[MCS_OPT_K1_WS] == 1 && v[MCS_OPT_TAIL_LOOP] == 6 && v[MCS_OPT_DEFER_K] == 3 && v[MCS_OPT_PARK] == 0);
  // use_env = 0: nothing of the shell
  CHECK(mcs_options_resolve(keys, vals, 4, false, 0, v, &msg) == MCS_OPTION_OK);
  CHECK(v[MCS_OPT_FORCE_GENERAL] == 0 && v[MCS_OPT_K1_WS] == 1 && v[MCS_OPT_TAIL_LOOP] == 6);
  for (int k = 0; k < MCS_OPT_COUNT; ++k) if (k != MCS_OPT_K1_WS && k != MCS_OPT_TAIL_LOOP) CHECK(v[k] == kMcsOptions[k].dflt);
  clear_env();
}

static void test_refusals() {
  std::string msg;
  int64_t v[MCS_OPT_COUNT];
  // unknown keys
  for (int key : {-1, (int)MCS_OPT_COUNT, 99}) {
    msg.clear();
    CHECK(mcs_option_check(key, 0, 0, &msg) == MCS_OPTION_UNKNOWN && has(msg, "unknown option key") && has(msg, std::to_string(key).c_str()));
    CHECK(mcs_option_check_set(key, 0, 0, false, &msg) == MCS_OPTION_UNKNOWN);
  }
  CHECK(mcs_option_check(99, 0, 0, nullptr) == MCS_OPTION_UNKNOWN);      // (a message is optional)
  // every key: its bounds hold, one past either is refused with name and range
  for (const McsOptionRow& r : kMcsOptions) {
    const int fp32 = r.applies == MCS_APPLIES_FP32;
    CHECK(mcs_option_check(r.key, r.min, fp32, &msg) == MCS_OPTION_OK);
    CHECK(mcs_option_check(r.key, r.max, fp32, &msg) == MCS_OPTION_OK);
    msg.clear();
    CHECK(mcs_option_check(r.key, r.min - 1, fp32, &msg) == MCS_OPTION_RANGE);
    CHECK(has(msg, r.name) && has(msg, (std::to_string(r.min) + ".." + std::to_string(r.max)).c_str()));
    if (r.max < INT64_MAX) CHECK(mcs_option_check(r.key, r.max + 1, fp32, &msg) == MCS_OPTION_RANGE);
  }
  msg.clear();
  CHECK(mcs_option_check(MCS_OPT_DEFER_K, 99, 0, &msg) == MCS_OPTION_RANGE && has(msg, "defer_k") && has(msg, "MCS_OPT_DEFER_K") && has(msg, "1..40") && has(msg, "99"));
  // fp32 keys on a fp64 context, whatever the value; fine on a fp32 one
  for (int key : {MCS_OPT_F32_LOOP, MCS_OPT_F32_EXACT}) {
    msg.clear();
    CHECK(mcs_option_check(key, 1, 0, &msg) == MCS_OPTION_APPLIES && has(msg, kMcsOptions[key].name) && has(msg, "fp32"));
    CHECK(mcs_option_check(key, 0, 0, &msg) == MCS_OPTION_APPLIES);
    CHECK(mcs_option_check(key, 1, 1, &msg) == MCS_OPTION_OK && mcs_option_check_set(key, 1, 1, true, &msg) == MCS_OPTION_OK);
  }
  // a tail budget above 0 on a fp32-state context
  msg.clear();
  CHECK(mcs_option_check(MCS_OPT_TAIL_BUDGET, 4, 1, &msg) == MCS_OPTION_APPLIES && has(msg, "tail_budget") && has(msg, "fp64"));
  CHECK(mcs_option_check(MCS_OPT_TAIL_BUDGET, 0, 1, &msg) == MCS_OPTION_OK && mcs_option_check(MCS_OPT_TAIL_BUDGET, 4, 0, &msg) == MCS_OPTION_OK);
  // when: creation only; before the first pipelined run
  msg.clear();
  CHECK(mcs_option_check(MCS_OPT_TALLY_REPLICAS, 0, 0, &msg) == MCS_OPTION_OK);
  CHECK(mcs_option_check_set(MCS_OPT_TALLY_REPLICAS, 0, 0, false, &msg) == MCS_OPTION_WHEN && has(msg, "tally_replicas") && has(msg, "creation"));
  CHECK(mcs_option_check_set(MCS_OPT_TALLY_REPLICAS, 2, 0, false, &msg) == MCS_OPTION_RANGE);      // (the range comes first)
  CHECK(mcs_option_check_set(MCS_OPT_PIPE_SIDE_CUS, 0, 0, false, &msg) == MCS_OPTION_OK);
  msg.clear();
  CHECK(mcs_option_check_set(MCS_OPT_PIPE_SIDE_CUS, 0, 0, true, &msg) == MCS_OPTION_WHEN && has(msg, "pipe_side_cus") && has(msg, "pipelined"));
  for (const McsOptionRow& r : kMcsOptions)
    if (r.when == MCS_WHEN_BETWEEN_LAUNCHES) CHECK(mcs_option_check_set(r.key, r.dflt, r.applies == MCS_APPLIES_FP32, true, &msg) == MCS_OPTION_OK);
  // lists: one bad pair refuses the list, the environment never does
  {
    const int32_t keys[] = {MCS_OPT_PARK, 99};
    const int64_t vals[] = {0, 0};
    msg.clear();
    CHECK(mcs_options_resolve(keys, vals, 2, false, 0, v, &msg) == MCS_OPTION_UNKNOWN && has(msg, "99"));
    CHECK(mcs_options_resolve(keys, vals, 1, false, 0, v, &msg) == MCS_OPTION_OK && v[MCS_OPT_PARK] == 0);
  }
  {
    const int32_t keys[] = {MCS_OPT_DEFER_K};
    const int64_t vals[] = {99};
    CHECK(mcs_options_resolve(keys, vals, 1, true, 0, v, &msg) == MCS_OPTION_RANGE && has(msg, "defer_k") && has(msg, "1..40"));
    const int32_t k2[] = {MCS_OPT_F32_EXACT};
    const int64_t v2[] = {1};
    CHECK(mcs_options_resolve(k2, v2, 1, true, 0, v, &msg) == MCS_OPTION_APPLIES && has(msg, "f32_exact"));
    CHECK(mcs_options_resolve(k2, v2, 1, true, 1, v, &msg) == MCS_OPTION_OK && v[MCS_OPT_F32_EXACT] == 1);
    const int32_t k3[] = {MCS_OPT_TAIL_BUDGET};
    const int64_t v3[] = {4};
    CHECK(mcs_options_resolve(k3, v3, 1, true, 1, v, &msg) == MCS_OPTION_APPLIES && has(msg, "tail_budget"));
    CHECK(mcs_options_resolve(k3, v3, 1, true, 0, v, &msg) == MCS_OPTION_OK && v[MCS_OPT_TAIL_BUDGET] == 4);
  }
  msg.clear();
  CHECK(mcs_options_resolve(nullptr, nullptr, 1, false, 0, v, &msg) != MCS_OPTION_OK && has(msg, "null"));
  CHECK(mcs_options_resolve(nullptr, nullptr, -1, false, 0, v, &msg) != MCS_OPTION_OK);
  put("MCS_DEFER_K", "99"); put("MCS_TAIL_BUDGET", "4");
  CHECK(mcs_options_resolve(nullptr, nullptr, 0, true, 1, v, &msg) == MCS_OPTION_OK && v[MCS_OPT_DEFER_K] == 8 && v[MCS_OPT_TAIL_BUDGET] == 4);
  clear_env();
}

int main() {
  test_table();
  test_env_rules();
  test_precedence();
  test_refusals();
  if (g_fail) { std::printf("%d check(s) failed\n", g_fail); return 1; }
  std::printf("OPTIONS_OK\n");
  return 0;
}
