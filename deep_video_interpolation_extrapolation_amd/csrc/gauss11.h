// The 11-tap gaussian window (sigma 1.5) of the SSIM kernels (score.hip, msssim.hip).
#pragma once

namespace dvie {

// exp(-(k - 5)^2 / (2 * 1.5^2)) / sum, in float64 (losses.py:18-20 under a float64 default)
__host__ __device__ __forceinline__ constexpr double sc_g(int k) {
  const int d = k < 5 ? 5 - k : k - 5;
  return d == 0 ? 0.26601172486179436
       : d == 1 ? 0.2130055377112537
       : d == 2 ? 0.10936068950970002
       : d == 3 ? 0.03600077212843083
       : d == 4 ? 0.007598758135239185
                : 0.00102838008447911;
}

}  // namespace dvie
