// The one place libupsparts_hip.so parses an environment switch (the table of all of them: ../switches.py).
// Four parse rules, each in two flavours that a call site names:
//   ups_env_on_now(name)   / UPS_ENV_ON_CACHED(name)       default-on:  off only when the value starts with '0'
//   ups_env_off_now(name)  / UPS_ENV_OFF_CACHED(name)      default-off: on only when the value starts with '1'
//   ups_env_int_now(n, d)  / UPS_ENV_INT_CACHED(n, d)      atoll of the value, `d` when the switch is unset
//   ups_env_raw_now(name)  / UPS_ENV_RAW_CACHED(name)      the string itself (nullptr when unset)
// `_now` reads the environment at every call: the switches that tests toggle inside one process.  `_CACHED` reads it once per
// process and call site (a function-local static: thread-safe initialisation) -- a later setenv is not seen.  Which of the two a
// switch uses is part of its contract: a test that toggles a cached switch silently exercises one form twice.
#pragma once
#include <stdlib.h>

static inline const char* ups_env_raw_now(const char* name) { return getenv(name); }
static inline bool ups_env_on_now(const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); }
static inline bool ups_env_off_now(const char* name) { const char* e = getenv(name); return e && e[0] == '1'; }
// (a site that wants an int casts: on LP64 (int)atoll(e) and atoi(e) are the same truncation of the same strtol)
static inline long long ups_env_int_now(const char* name, long long dflt) { const char* e = getenv(name); return e ? atoll(e) : dflt; }

#define UPS_ENV_CACHED_(expr) ([] { static const auto v_ = (expr); return v_; }())
#define UPS_ENV_ON_CACHED(name) UPS_ENV_CACHED_(ups_env_on_now(name))
#define UPS_ENV_OFF_CACHED(name) UPS_ENV_CACHED_(ups_env_off_now(name))
#define UPS_ENV_INT_CACHED(name, dflt) UPS_ENV_CACHED_(ups_env_int_now(name, dflt))
#define UPS_ENV_RAW_CACHED(name) UPS_ENV_CACHED_(ups_env_raw_now(name))
