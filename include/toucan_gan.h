/*
 * toucan_gan.h - C ABI of the speaker-embedding GAN in libtoucan_hip.so: the generator ResNet_G of the reference's
 * InferenceInterfaces/Controllability/wgan/resnet_1.py (:8-80, ResNetBlock :133-181), which GanWrapper (Controllability/GAN.py) and
 * ControllableInterface drive.  Same conventions as toucan_tts.h (device pointers owned by the caller, one hipStream_t per call,
 * 0 or a negative TTS_E_* code, tts_last_error()).  The only caller is the build's own Python host (ims-toucan-prosody-variance_amd/
 * gan.py, via ctypes: capi.GAN_PROTOTYPES).
 *
 * Every layer of the generator is one launch of tts_gan_conv2d: the 3x3 and 1x1 convolutions at their image size, and the two
 * Linear layers (fc, fc_out) as 1x1 convolutions of 1x1 images.  fp32 only.
 */
#ifndef TOUCAN_GAN_H
#define TOUCAN_GAN_H

#include "toucan_tts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* packing of the weights: w[taps][cin_pad][cout_pad], cin_pad = cin rounded up to TTS_GAN_KC, cout_pad = cout rounded up to
 * TTS_GAN_NC, zero outside [cin) x [cout).  Tap t = 3 * ky + kx of the torch kernel [cout][cin][ky][kx]. */
#define TTS_GAN_KC 16
#define TTS_GAN_NC 64

/* flags of TtsGanConvDesc */
#define TTS_GAN_UPSAMPLE 1     /* x is [n][h/2][h/2][cin], read through a nearest x2 upsample (nn.Upsample(scale_factor=2))        */
#define TTS_GAN_PRE_LRELU 2    /* LeakyReLU(pre_slope) on every element of x as it is loaded (the zero padding stays 0)               */
#define TTS_GAN_RESIDUAL 4     /* out = act(res + res_ratio * v)                                                                     */
#define TTS_GAN_RES_UPSAMPLE 8 /* res is [n][h/2][h/2][cout], read through the same upsample (an identity shortcut after Upsample) */
#define TTS_GAN_LRELU 16       /* act = LeakyReLU(slope); without it act is the identity                                           */

/* One convolution over a batch of n square h x h images, NHWC fp32, stride 1, zero padding (taps 9: 3x3, padding 1; taps 1: 1x1):
 *   v[p][co]   = scale[co] * sum_{t, ci} w[t][ci][co] * pre(x[p + offset(t)][ci]) + shift[co]   (scale null: 1, shift null: 0)
 *   y[p][co]   = act(v) or, with TTS_GAN_RESIDUAL, act(res[p][co] + res_ratio * v)
 * An implicit GEMM on the fp32 matrix cores (v_mfma_f32_32x32x2_f32): M = n*h*h pixels, N = cout, K = taps*cin_pad.  A tile of 64
 * pixels spans several images when h*h < 64; the padding is taken at the image's edges.  Every output is one k-ordered fp32 fma
 * chain over (t, ci) whatever n and the pixel's place in the batch, so an image comes out bit for bit the same alone or in any
 * batch.  y must not overlap x or res. */
typedef struct TtsGanConvDesc {
  const float* x;
  const float* w;
  const float* scale;
  const float* shift;
  const float* res;
  float* y;
  int32_t n, h, cin, cout, taps;
  int32_t flags;
  float pre_slope, res_ratio, slope;
} TtsGanConvDesc;

int tts_gan_conv2d(const TtsGanConvDesc* d, tts_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TOUCAN_GAN_H */
