// Checks of dla::Knob (csrc/include/dla_knob.h), the one type behind every DLA_* switch of the native code, as a
// standalone executable that runs under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU beside host_check:
// every parse form against the values unset, "", 0, 1, 00, off, 7, -3 and abc; override, clear and override again;
// that the environment is read once; and the cap of APPLY_MAX_K. Each case sets the environment with setenv and
// then constructs a fresh instance.
//
// Build + run: python -m distributed_learning_amd._build --sanitize   (g++ -fsanitize=address,undefined)
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../include/dla_knob.h"

using dla::Knob;

namespace {

int g_cases = 0, g_fail = 0;

void check(bool ok, const std::string& what) {
  ++g_cases;
  if (!ok) {
    ++g_fail;
    std::fprintf(stderr, "FAIL %s\n", what.c_str());
  }
}

// nullptr unsets DLA_CHECK; the knobs under test are all named CHECK
void env(const char* v) {
  if (v) setenv("DLA_CHECK", v, 1);
  else unsetenv("DLA_CHECK");
}

constexpr int kValues = 9;
const char* const kEnv[kValues] = {nullptr, "", "0", "1", "00", "off", "7", "-3", "abc"};

void expect(const char* form, Knob (*make)(), const double (&want)[kValues]) {
  for (int i = 0; i < kValues; ++i) {
    env(kEnv[i]);
    Knob k = make();
    const std::string what = std::string(form) + " with DLA_CHECK=" + (kEnv[i] ? "'" + std::string(kEnv[i]) + "'" : "unset");
    check(k.real_value() == want[i], what + ": got " + std::to_string(k.real_value()));
    check(k.value() == (int)want[i] && k.on() == (want[i] != 0) && !k.overridden(), what + ": value / on / overridden");
  }
}

void parse_forms() {
  //                                                       unset  ""  0  1  00  off  7  -3  abc
  expect("on_unless_0", [] { return Knob::on_unless_0("CHECK"); }, {1, 1, 0, 1, 0, 1, 1, 1, 1});
  expect("off_unless_1", [] { return Knob::off_unless_1("CHECK"); }, {0, 0, 0, 1, 0, 0, 0, 0, 0});
  // atoi, the default only when unset: HALO (2), HALO_V (3), POOL3_SEP (4), CONV_PIPE (-1)
  expect("integer 2", [] { return Knob::integer("CHECK", 2); }, {2, 0, 0, 1, 0, 0, 7, -3, 0});
  expect("integer -1", [] { return Knob::integer("CHECK", -1); }, {-1, 0, 0, 1, 0, 0, 7, -3, 0});
  // GEMM_PERSIST: clamped to >= 0
  expect("integer 0 floor 0", [] { return Knob::integer("CHECK", 0, 0); }, {0, 0, 0, 1, 0, 0, 7, 0, 0});
  // the default when unset or <= 0: SPLITK_BLOCKS (512), BN_RED_BLOCKS (1024), TILE256_MIN_K_STATS (256)
  expect("positive 512", [] { return Knob::positive("CHECK", 512); }, {512, 512, 512, 1, 512, 512, 7, 512, 512});
  // APPLY_MAX_K: capped (the default is not)
  expect("positive 512 cap 4", [] { return Knob::positive("CHECK", 512, 4); }, {512, 512, 512, 1, 512, 512, 4, 512, 512});
  // COMM_TIMEOUT_S: atof
  expect("real 600", [] { return Knob::real("CHECK", 600.0); }, {600, 0, 0, 1, 0, 0, 7, -3, 0});
  env("2.5");
  Knob t = Knob::real("CHECK", 600.0);
  check(t.real_value() == 2.5, "real keeps the fraction");
}

// set / clear / set again: a cleared knob is back at the environment's value, not at the literal default
void overrides() {
  env("0");
  Knob on = Knob::on_unless_0("CHECK");
  check(!on.on() && !on.overridden(), "on_unless_0: environment 0");
  on.set(1);
  check(on.on() && on.overridden(), "on_unless_0: set(1) forces on");
  on.set(5);
  check(on.value() == 1, "on_unless_0: set(5) is on, value 1");
  on.set(0);
  check(!on.on() && on.overridden(), "on_unless_0: set(0) forces off");
  on.set(-1);
  check(!on.on() && !on.overridden(), "on_unless_0: set(-1) returns to the environment's 0");
  on.set(1);
  check(on.on() && on.overridden(), "on_unless_0: override again");
  on.clear();
  check(!on.on() && !on.overridden(), "on_unless_0: clear()");

  env("1");
  Knob off = Knob::off_unless_1("CHECK");
  off.set(0);
  check(!off.on() && off.overridden(), "off_unless_1: set(0) over environment 1");
  off.set(-1);
  check(off.on() && !off.overridden(), "off_unless_1: set(-1) returns to the environment's 1");

  env("3");
  Knob persist = Knob::integer("CHECK", 0, 0);
  persist.set(0);
  check(persist.value() == 0 && persist.overridden(), "integer: set(0) is an override");
  persist.set(2);
  check(persist.value() == 2, "integer: set(2)");
  persist.set(-1);
  check(persist.value() == 3 && !persist.overridden(), "integer: set(-1) returns to the environment's 3");

  env("384");
  Knob pos = Knob::positive("CHECK", 256);
  pos.set(1024);
  check(pos.value() == 1024 && pos.overridden(), "positive: set(1024)");
  pos.set(-1);
  check(pos.value() == 384 && !pos.overridden(), "positive: set(-1) returns to the environment's 384");
  pos.set(64);
  pos.set(0);
  check(pos.value() == 384 && !pos.overridden(), "positive: set(0) returns to the environment's 384");
  env(nullptr);
  Knob def = Knob::positive("CHECK", 256);
  def.set(64);
  def.set(-1);
  check(def.value() == 256, "positive: set(-1) with the variable unset returns to the default");
}

void cap() {
  env("4096");
  Knob k = Knob::positive("CHECK", 512, 2048);
  check(k.value() == 2048, "APPLY_MAX_K form: the environment's value is capped");
  k.set(100000);
  check(k.value() == 2048 && k.overridden(), "APPLY_MAX_K form: an override is capped");
  k.set(1024);
  check(k.value() == 1024, "APPLY_MAX_K form: an override below the cap stands");
  k.set(0);
  check(k.value() == 2048 && !k.overridden(), "APPLY_MAX_K form: cleared, back at the (capped) environment");
}

// the environment is read on first use, and only then
void read_once() {
  env("0");
  Knob lazy = Knob::on_unless_0("CHECK");
  env("1");
  check(lazy.on(), "read lazily: the value at first use counts, not at construction");
  env("0");
  check(lazy.on(), "read once: a later change of the environment is not seen");
  lazy.set(0);
  lazy.set(-1);
  check(lazy.on(), "read once: clearing an override does not read again");

  env("5");
  Knob early = Knob::integer("CHECK", 2);
  early.set(9);  // an override before the first read does not stop the read that clear() needs
  env("6");
  check(early.value() == 9, "override before the first read");
  early.clear();
  check(early.value() == 6, "first read after clear()");
}

}  // namespace

int main() {
  parse_forms();
  overrides();
  cap();
  read_once();
  std::printf("knob_check: %d cases, %d failed\n", g_cases, g_fail);
  return g_fail ? 1 : 0;
}
