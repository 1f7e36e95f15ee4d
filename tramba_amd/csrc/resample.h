// Host-side tables of Pillow's 8-bit resampler, shared by the frame pipeline (frames.hip) and the training augmentation
// (augment.hip).  Built in fp64 with FP contraction off, as Pillow's Resample.c computes them.
#pragma once
#include "common.h"

namespace tramba {

constexpr int kPrecBits = 22;             // Pillow's fixed-point precision for 8-bit images

enum ResampleFilter { kFilterBilinear = 0, kFilterBicubic = 1 };

// Taps per output sample of one axis: ceil(support * max(in / out, 1)) * 2 + 1; an axis whose size does not change is a
// one-tap copy (weight 2^22).
int resample_taps(int in, int out, int filter);
// bounds[out][2] = {first input sample, taps used}, coef[out][ksize] fixed-point weights (22 fractional bits; a negative
// weight rounds as int(w 2^22 - 0.5), a positive one as int(w 2^22 + 0.5)).  False when a row needs more than ksize taps.
bool resample_axis(int in, int out, int filter, int ksize, int *bounds, int *coef);
// lut[3][256] = fp32(fp32(u / 255) - mean[c]) / std[c] with mean / std as fp64 operands (to_tensors' rounding)
void normalise_lut(const double *mean, const double *std, float *lut);
bool frame_sizes_ok(int in_h, int in_w, int out_h, int out_w);

}  // namespace tramba
