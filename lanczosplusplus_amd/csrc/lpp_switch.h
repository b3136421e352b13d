// lpp_switch.h -- an LPP_* environment switch as the planners see it (lpp_pb_plan.h, lpp_csr_plan.h): a value, never a getenv at the
// point of use.  Plain C++.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdlib>

namespace lpp {

// unset, or the integer it was set to
struct EnvSwitch {
	bool set = false;
	int v = 0;
	int value_or(int dflt) const { return set ? v : dflt; }
	bool off() const { return set && v == 0; } // "=0 switches it off"
};

// for the *_switches_from_env readers only
inline EnvSwitch env_switch(const char* name)
{
	EnvSwitch s;
	if (const char* t = getenv(name)) {
		s.set = true;
		s.v = (int)std::max<long long>(INT_MIN, std::min<long long>(atoll(t), INT_MAX));
	}
	return s;
}

} // namespace lpp
