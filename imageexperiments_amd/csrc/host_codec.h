// host_codec.h -- product host code: whole-image helpers around the decoded pixels.
//   psnr              compressed::calculatePSNR          CompressedImage.cpp:343-357
//   psnr_from_sse     its last two lines (mpc_rate_distortion: the sum comes from mp_distortion_kernel)
// Tile reconstruction (compressed::decodeImage / matching::FromCoeffsDynamic / img::RGBFromYUV) runs on the
// device only: mp_decode_kernel in mp_kernels.hip behind mpc_decode_image / mpc_decode_tiles_device.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mpc {

double psnr(const uint8_t* original, const uint8_t* decoded, int width, int height);
// the formula of calculatePSNR from its sum of squared differences (the sum is of integers: exact below 2^53)
double psnr_from_sse(double se, int width, int height);
// the same over `pixels` pixels: a group of frames' (psnr_from_sse is this at width * height)
double psnr_from_sse_pixels(double se, size_t pixels);

}  // namespace mpc
