// mcs_options.h -- the run options of a context (enum mcs_option of include/mcs.h): ONE table with a row per option -- key, name,
// the environment variable that seeds its default and the rule by which that variable is read, range, built-in default, when it may
// change and which contexts it applies to -- and the functions that work on the table: the three rules, the initial values of a
// context (built-in default < environment < the caller's list), the check of a (key, value) pair.  mcs_api.hip walks the table and
// names no variable itself.  Plain C++17 without a HIP include: a host compiler builds it alone, tests/native/options_main.cpp does.
#pragma once
#include "../../include/mcs.h"

#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

// ---- the environment: read once per context, at creation
// on iff the first character is '1'
inline bool env_on(const char* name) { const char* e = std::getenv(name); return e && e[0] == '1'; }
// off iff the first character is '0'
inline bool env_not_off(const char* name) { const char* e = std::getenv(name); return !(e && e[0] == '0'); }
// an integer inside lo..hi, else (unset, outside, not a number that lies inside) the default stays
inline long long env_int(const char* name, long long lo, long long hi, long long dflt) {
  const char* e = std::getenv(name);
  if (!e) return dflt;
  const long long v = std::atoll(e);
  return v >= lo && v <= hi ? v : dflt;
}
// '1' -> 1, '0' -> 0, anything else or unset -> 2
inline int env_tristate(const char* name) { const char* e = std::getenv(name); return !e ? 2 : (e[0] == '1' ? 1 : (e[0] == '0' ? 0 : 2)); }

// which of the rules reads a row's variable; inverted: the option is 1 - what env_on gives (MCS_TALLY_REPLICAS_OFF)
enum McsEnvRule { MCS_ENV_ON = 0, MCS_ENV_NOT_OFF, MCS_ENV_INT, MCS_ENV_TRISTATE, MCS_ENV_ON_INVERTED };

struct McsOptionRow {
  int32_t key;
  const char* name;
  const char* env;
  int32_t rule;             // McsEnvRule
  int64_t min, max, dflt;   // inclusive range of a caller's value (and of MCS_ENV_INT); built-in default
  int32_t when;             // enum mcs_option_when
  int32_t applies;          // enum mcs_option_applies
};

// (the largest budget mcs_set_tail_slicing has always taken)
constexpr int64_t kMcsTailBudgetMax = 1 << 24;

// Row k describes key k.
constexpr McsOptionRow kMcsOptions[MCS_OPT_COUNT] = {
    {MCS_OPT_FORCE_GENERAL, "force_general", "MCS_FORCE_GENERAL", MCS_ENV_ON, 0, 1, 0, MCS_WHEN_BETWEEN_LAUNCHES, MCS_APPLIES_ANY},
    {MCS_OPT_K1_WS, "k1_ws", "MCS_K1_WS", MCS_ENV_TRISTATE, 0, 2, 2, MCS_WHEN_BETWEEN_LAUNCHES, MCS_APPLIES_ANY},
    {MCS_OPT_WS_AUTO_MIN, "ws_auto_min", "MCS_WS_AUTO_MIN", MCS_ENV_INT, 0, INT64_MAX, 6000000, MCS_WHEN_BETWEEN_LAUNCHES, MCS_APPLIES_ANY},
    {MCS_OPT_TAIL_MERGE, "tail_merge", "MCS_TAIL_MERGE", MCS_ENV_NOT_OFF, 0, 1, 1, MCS_WHEN_BETWEEN_LAUNCHES, MCS_APPLIES_ANY},
    {MCS_OPT_PARK, "park", "MCS_PARK", MCS_ENV_NOT_OFF, 0, 1, 1, MCS_WHEN_BETWEEN_LAUNCHES, MCS_APPLIES_ANY},
    {MCS_OPT_TAIL_RING, "tail_ring", "MCS_TAIL_RING", MCS_ENV_NOT_OFF, 0, 1, 1, MCS_WHEN_BETWEEN_LAUNCHES, MCS_APPLIES_ANY},
    {MCS_OPT_TAIL_LOOP, "tail_loop", "MCS_TAIL_LOOP", MCS_ENV_INT, 0, 32, 12, MCS_WHEN_BETWEEN_LAUNCHES, MCS_APPLIES_ANY},
    {MCS_OPT_REFILL_MIN, "refill_min", "MCS_REFILL_MIN", MCS_ENV_INT, 1, 48, 12, MCS_WHEN_BETWEEN_LAUNCHES, MCS_APPLIES_ANY},
    {MCS_OPT_DEFER_K, "defer_k", "MCS_DEFER_K", MCS_ENV_INT, 1, 40, 8, MCS_WHEN_BETWEEN_LAUNCHES, MCS_APPLIES_ANY},
    {MCS_OPT_TAIL_BUDGET, "tail_budget", "MCS_TAIL_BUDGET", MCS_ENV_INT, 0, kMcsTailBudgetMax, 0, MCS_WHEN_BETWEEN_LAUNCHES, MCS_APPLIES_FP64_IF_POSITIVE},
    {MCS_OPT_PIPE_SIDE_CUS, "pipe_side_cus", "MCS_PIPE_SIDE_CUS", MCS_ENV_INT, 0, 128, 12, MCS_WHEN_BEFORE_PIPELINED_RUN, MCS_APPLIES_ANY},
    {MCS_OPT_TALLY_REPLICAS, "tally_replicas", "MCS_TALLY_REPLICAS_OFF", MCS_ENV_ON_INVERTED, 0, 1, 1, MCS_WHEN_CREATION, MCS_APPLIES_ANY},
    {MCS_OPT_F32_LOOP, "f32_loop", "MCS_F32_LOOP", MCS_ENV_ON, 0, 1, 0, MCS_WHEN_BETWEEN_LAUNCHES, MCS_APPLIES_FP32},
    {MCS_OPT_F32_EXACT, "f32_exact", "MCS_F32_EXACT", MCS_ENV_ON, 0, 1, 0, MCS_WHEN_BETWEEN_LAUNCHES, MCS_APPLIES_FP32},
};
constexpr bool mcs_options_in_key_order() {
  for (int k = 0; k < MCS_OPT_COUNT; ++k) if (kMcsOptions[k].key != k) return false;
  return true;
}
static_assert(mcs_options_in_key_order(), "row k of kMcsOptions must describe key k");

// the row of a key, null for a key that does not exist
inline const McsOptionRow* mcs_option_row(int key) { return key >= 0 && key < MCS_OPT_COUNT ? &kMcsOptions[key] : nullptr; }

// What the row's variable gives a new context: the value by the row's rule; the built-in default where the variable is unset (every
// rule) or holds no number inside the range (MCS_ENV_INT).  Whether the option applies to the context is not asked here, as it never
// was: a variable that does not apply is carried and has the effect it always had.
inline int64_t mcs_option_from_env(const McsOptionRow& r) {
  switch (r.rule) {
    case MCS_ENV_ON: return env_on(r.env) ? 1 : 0;
    case MCS_ENV_ON_INVERTED: return env_on(r.env) ? 0 : 1;
    case MCS_ENV_NOT_OFF: return env_not_off(r.env) ? 1 : 0;
    case MCS_ENV_TRISTATE: return env_tristate(r.env);
    default: return env_int(r.env, r.min, r.max, r.dflt);
  }
}

// ---- a caller's (key, value): why it is refused, with a message that names the option and what it allows
enum McsOptionRefusal { MCS_OPTION_OK = 0, MCS_OPTION_UNKNOWN, MCS_OPTION_RANGE, MCS_OPTION_APPLIES, MCS_OPTION_WHEN };

inline std::string mcs_option_label(const McsOptionRow& r) {
  std::string up;
  for (const char* p = r.name; *p; ++p) up += (char)(*p >= 'a' && *p <= 'z' ? *p - 'a' + 'A' : *p);
  return std::string("option ") + r.name + " (MCS_OPT_" + up + ")";
}

// a value for a context with fp64 (state_fp32 == 0) or fp32 particle state, at creation
inline McsOptionRefusal mcs_option_check(int key, int64_t value, int state_fp32, std::string* msg) {
  const McsOptionRow* r = mcs_option_row(key);
  char b[160];
  if (!r) {
    std::snprintf(b, sizeof b, "unknown option key %d (the keys are 0..%d, enum mcs_option)", key, MCS_OPT_COUNT - 1);
    if (msg) *msg = b;
    return MCS_OPTION_UNKNOWN;
  }
  if (value < r->min || value > r->max) {
    std::snprintf(b, sizeof b, ": value %lld outside its range %lld..%lld", (long long)value, (long long)r->min, (long long)r->max);
    if (msg) *msg = mcs_option_label(*r) + b;
    return MCS_OPTION_RANGE;
  }
  if (r->applies == MCS_APPLIES_FP32 && !state_fp32) {
    if (msg) *msg = mcs_option_label(*r) + ": only for a context with fp32 particle state (mcs_params.state_fp32 = 1)";
    return MCS_OPTION_APPLIES;
  }
  if (r->applies == MCS_APPLIES_FP64_IF_POSITIVE && value > 0 && state_fp32) {
    if (msg) *msg = mcs_option_label(*r) + ": a value above 0 only for a context with fp64 particle state (mcs_params.state_fp32 = 0)";
    return MCS_OPTION_APPLIES;
  }
  return MCS_OPTION_OK;
}

// ... for a context that exists (mcs_set_option); pipelined_run_made: the context has made its first pipelined run
inline McsOptionRefusal mcs_option_check_set(int key, int64_t value, int state_fp32, bool pipelined_run_made, std::string* msg) {
  const McsOptionRefusal why = mcs_option_check(key, value, state_fp32, msg);
  if (why != MCS_OPTION_OK) return why;
  const McsOptionRow& r = kMcsOptions[key];
  if (r.when == MCS_WHEN_CREATION) {
    if (msg) *msg = mcs_option_label(r) + ": set at creation only (mcs_create_with_options)";
    return MCS_OPTION_WHEN;
  }
  if (r.when == MCS_WHEN_BEFORE_PIPELINED_RUN && pipelined_run_made) {
    if (msg) *msg = mcs_option_label(r) + ": fixed by the context's first pipelined run";
    return MCS_OPTION_WHEN;
  }
  return MCS_OPTION_OK;
}

// The values a new context starts with, into out[MCS_OPT_COUNT]: the built-in defaults, then the environment (use_env), then the
// caller's n pairs in their order (a key given twice: the last one).  One bad pair refuses the list: the message says which.
inline McsOptionRefusal mcs_options_resolve(const int32_t* keys, const int64_t* values, int n, bool use_env, int state_fp32, int64_t* out,
                                            std::string* msg) {
  if (n < 0 || (n > 0 && (!keys || !values))) {
    if (msg) *msg = "option list: n_options < 0, or null keys / values with n_options > 0";
    return MCS_OPTION_UNKNOWN;
  }
  for (int k = 0; k < MCS_OPT_COUNT; ++k) out[k] = use_env ? mcs_option_from_env(kMcsOptions[k]) : kMcsOptions[k].dflt;
  for (int i = 0; i < n; ++i) {
    const McsOptionRefusal why = mcs_option_check(keys[i], values[i], state_fp32, msg);
    if (why != MCS_OPTION_OK) return why;
    out[keys[i]] = values[i];
  }
  return MCS_OPTION_OK;
}
