// lpp_launch.h -- what the host side of every kernel launch shares: the grid rule, runtime flags as template arguments, and the launch
// of a kernel with dynamic LDS through its pointer.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

namespace lpp {

// `units` of work over the CUs, at most per_cu workgroups each; from 8 on a multiple of 8, so that every XCD gets the same number
// (and the XCD-contiguous mappings of the kernels apply)
inline int launch_grid(int64_t units, int num_cus, int per_cu = 1)
{
	const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(units, (int64_t)num_cus * per_cu));
	return nb >= 8 ? nb & ~7 : nb;
}

// f(std::bool_constant<flags>...): runtime flags as integral constants for a generic lambda, which names its template instance with them
template <typename F> void with_flags(F&& f) { f(); }
template <typename F, typename... Rest> void with_flags(F&& f, bool flag, Rest... rest)
{
	if (flag) with_flags([&](auto... c) { f(std::true_type {}, c...); }, rest...);
	else with_flags([&](auto... c) { f(std::false_type {}, c...); }, rest...);
}

// a kernel that sizes its dynamic LDS beyond the default 64 KB.  The attribute is set at every launch: it belongs to the function and
// the device, and two engines may ask for different sizes
template <typename Args> void launch_lds(void (*kernel)(Args), int grid, int threads, size_t lds_bytes, hipStream_t st, const Args& args)
{
	(void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
	kernel<<<grid, threads, lds_bytes, st>>>(args);
}

} // namespace lpp
