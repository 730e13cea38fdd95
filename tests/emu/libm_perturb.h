// Test-only: force-included (-include) into every source of _build/libemu_libm.so.  Declares wo::tanh, exp, sin, cos, atan2,
// pow and asin, so that the unqualified calls inside namespace wo (the kernel bodies of elevation_ops.h and the other *_ops.h)
// resolve to the wrappers of libm_perturb.cc instead of glibc's.  Qualified calls (std::pow in the host stage, which runs on the
// host in the product as well) keep glibc's.  The wrappers return glibc's result moved by k double ulps (emu_set_libm_perturb).
#pragma once
#include <cmath>

namespace wo {
double tanh(double x);
double exp(double x);
double sin(double x);
double cos(double x);
double atan2(double y, double x);
double pow(double x, double y);
double asin(double x);
}  // namespace wo
