// One environment switch (DLA_<NAME>) with an optional run-time override: the only place the native code
// reads a DLA_* variable. Every A/B switch is one declaration of this type, with its name and default as
// literals (tests/test_knobs.py scans them against distributed_learning_amd/knobs.py):
//
//   static Knob k_tn256 = Knob::on_unless_0("TN256");
//   void set_tn256(int mode) { k_tn256.set(mode); }        // a set_* function bound into _C
//   ... k_tn256.on() ...
//
// The environment is read once, on first use. set() installs an override or, given the form's "none" value,
// clears it; a cleared knob is back at its environment-or-default value, whatever the form.
#pragma once

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <mutex>
#include <string>

namespace dla {

class Knob {
 public:
  // on unless the value starts with '0'; set(mode): < 0 clears, 0 off, else on
  static Knob on_unless_0(const char* name) { return Knob(name, kOnUnless0, 1, 0, 0); }
  // off unless the value starts with '1'; set(mode): < 0 clears, 0 off, else on
  static Knob off_unless_1(const char* name) { return Knob(name, kOffUnless1, 0, 0, 0); }
  // atoi of the value (at least `floor`), `def` when unset; set(v): < 0 clears
  static Knob integer(const char* name, int def, int floor = INT_MIN) { return Knob(name, kInteger, def, floor, 0); }
  // atoi of the value (at most `cap`), `def` when unset or <= 0; set(v): <= 0 clears
  static Knob positive(const char* name, int def, int cap = INT_MAX) { return Knob(name, kPositive, def, 0, cap); }
  // atof of the value, `def` when unset
  static Knob real(const char* name, double def) { return Knob(name, kReal, def, 0, 0); }

  void set(int v) {
    if (form_ == kPositive ? v <= 0 : v < 0) return clear();
    overridden_ = true;
    override_ = form_ == kPositive ? std::min(v, hi_) : form_ == kInteger ? v : (v != 0);
  }
  void clear() { overridden_ = false; }
  bool overridden() const { return overridden_; }  // value() is then what set() installed

  int value() const { return (int)real_value(); }
  bool on() const { return value() != 0; }
  double real_value() const { return overridden_ ? override_ : env(); }

 private:
  enum Form { kOnUnless0, kOffUnless1, kInteger, kPositive, kReal };
  Knob(const char* name, Form form, double def, int lo, int hi)
      : name_(name), form_(form), def_(def), lo_(lo), hi_(hi) {}

  double env() const {
    std::call_once(once_, [this] { env_ = parse(std::getenv((std::string("DLA_") + name_).c_str())); });
    return env_;
  }
  double parse(const char* e) const {
    switch (form_) {
      case kOnUnless0: return !(e && e[0] == '0');
      case kOffUnless1: return e && e[0] == '1';
      case kInteger: return e ? std::max(lo_, std::atoi(e)) : def_;
      case kPositive: {
        const int v = e ? std::atoi(e) : 0;
        return v > 0 ? std::min(v, hi_) : def_;
      }
      default: return e ? std::atof(e) : def_;
    }
  }

  const char* name_;
  Form form_;
  double def_;
  int lo_, hi_;
  bool overridden_ = false;
  int override_ = 0;
  mutable std::once_flag once_;
  mutable double env_ = 0;
};

}  // namespace dla
