// fft_launch.h — what host code needs to launch a transform: the step from an FFT size known at run time to a kernel
// instantiation, the shape of a size without one, the twiddle table on the device, and the forward transform of real rows that
// every unit with filters to transform shares (defined in api_conv.hip, the FFT unit: k_spectrum_real is instantiated there only).
#pragma once
#include <type_traits>

#include "common.h"
#include "fft_lds.h"

namespace earhip {

// fixed(std::integral_constant<int, LL>{}) for L == LL, one of the powers of two MinL ... 8192 (the sizes with a kernel
// instantiation of their own); rt() for every other L (mixed radix at run time, or the caller's refusal)
template <int MinL, int LL = MinL, typename Fixed, typename Rt>
void fft_size_switch(int L, Fixed &&fixed, Rt &&rt) {
  if constexpr (LL > 8192) rt();
  else if (L == LL) fixed(std::integral_constant<int, LL>{});
  else fft_size_switch<MinL, 2 * LL>(L, fixed, rt);
}

// the passes of a size for the run-time kernels; `refusal`: what a caller with a size limit of its own says instead
inline FftShape shape_of(int L, const char *refusal = "FFT size must be in [4, 8192]") {
  FftShape S;
  if (!fft_make_shape(L, &S)) fail_invalid(refusal);
  return S;
}

// twiddle table exp(-2*pi*i*t/L), computed in double
std::vector<cf> make_twiddles(int L);
// ... made and copied into `tw` (allocated here; a blocking copy)
void upload_twiddles(DevBuf<cf> &tw, int L);

// out[row] = DFT_L of in[row][0 .. n_valid) zero-padded to L, rows `stride` floats apart
void launch_spectrum(int L, const float *in, size_t stride, int n_valid, const cf *tw, cf *out, int rows, hipStream_t s);

}  // namespace earhip
