// so3_dispatch.h -- run-time values to template arguments, and the name of the instantiation they pick.  Plain C++17, no HIP:
// so3proj.hip's launchers use it, tests/host_model/dispatch.cpp compiles it for the host.
//
//   with_flags([&](auto A, auto B) { launch(k<A(), B()>); }, a, b);       f(std::bool_constant<a>{}, std::bool_constant<b>{})
//   with_value<4, 2, 1>(u, [&](auto U) { launch(k<U()>); });              f(std::integral_constant<int, u>{}); false when u is not listed
//   kernel_label(buf, sizeof buf, "k", A, U);                             "k<true, 4>"
//
// Every combination of the flags (every listed value) instantiates the callable: one that can never be reached is left out with
// `if constexpr` inside it.  A nested lambda reads an outer constant through a `constexpr` local, not through the captured parameter.
#pragma once
#include <stddef.h>
#include <stdio.h>

#include <type_traits>

namespace so3 {

template <class F>
inline void with_flags(F &&f) { f(); }
// The constants reach f in the order of the flags.
template <class F, class... Rest>
inline void with_flags(F &&f, bool first, Rest... rest) {
    if (first) with_flags([&](auto... r) { f(std::true_type{}, r...); }, rest...);
    else with_flags([&](auto... r) { f(std::false_type{}, r...); }, rest...);
}

template <int... Vs, class F>
inline bool with_value(int v, F &&f) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// What is left of the buffer; a piece that does not fit is cut, the last byte stays free for the terminator.
struct LabelOut {
    char *p, *end;
    void put(const char *s) { while (*s != 0 && p < end) *p++ = *s++; }
    void put(bool v) { put(v ? "true" : "false"); }
    void put(int v) { char d[12]; snprintf(d, sizeof d, "%d", v); put(d); }
};

// "name<a, b, c>" as a profiler prints the instantiation: booleans as true / false, integers in decimal; the bare name without
// arguments.  Takes plain values and the constants with_flags / with_value hand out alike.  Returns buf (n > 0).
template <class... Args>
inline const char *kernel_label(char *buf, size_t n, const char *name, Args... args) {
    LabelOut out{buf, buf + n - 1};
    out.put(name);
    if constexpr (sizeof...(Args) > 0) {
        const char *sep = "<";
        ((out.put(sep), out.put(args), sep = ", "), ...);
        out.put(">");
    }
    *out.p = 0;
    return buf;
}

}  // namespace so3
