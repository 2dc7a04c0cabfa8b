// The speaker-embedding GAN's generator (InferenceInterfaces/Controllability/wgan/resnet_1.py, ResNet_G :8-80, ResNetBlock :133-181):
// one fused 2-D convolution entry, tts_gan_conv2d (include/toucan_gan.h), through which the host (gan.py) runs every layer.
//
// Implicit GEMM on the exact-fp32 matrix cores: M = n*h*h output pixels (NHWC rows), N = cout, K = taps * cin_pad in the order
// (tap, input channel).  A workgroup of four waves owns a 64-pixel x 64-channel tile, each wave a 32 x 32 quarter of it on
// v_mfma_f32_32x32x2_f32.  The K loop takes TTS_GAN_KC input channels of one tap per step: every thread loads four values of the
// pixel tile (the zero padding, the x2 upsample and the LeakyReLU applied as they are loaded) and four of the weight tile into
// registers one step ahead, and stores them to LDS (the pixel tile k-major, so the MFMA operands are read without bank conflicts).
//
// Batch independence: the accumulation order of an output is the fixed (tap, channel) order of K, whatever the tile, n or the pixel's
// place in the batch; the epilogue is element-wise.  No atomics, no split K.
#include "common.h"
#include "../../include/toucan_gan.h"

namespace tts {

constexpr int GAN_BM = 64, GAN_BN = TTS_GAN_NC, GAN_KC = TTS_GAN_KC, GAN_THREADS = 256, GAN_APAD = 4;
static_assert(GAN_BM * GAN_KC == 4 * GAN_THREADS && GAN_KC * GAN_BN == 4 * GAN_THREADS, "one float4 of each tile per thread");

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

__global__ __launch_bounds__(GAN_THREADS) void gan_conv2d_kernel(const TtsGanConvDesc d, const int cin_pad, const int cout_pad,
                                                                 const int M) {
  __shared__ __align__(16) float As[GAN_KC][GAN_BM + GAN_APAD];  // pixel tile, k-major
  __shared__ __align__(16) float Bs[GAN_KC][GAN_BN];             // weight tile
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int m0 = blockIdx.x * GAN_BM, n0 = blockIdx.y * GAN_BN;
  const int h = d.h, hw = h * h, cin = d.cin;
  const bool up = (d.flags & TTS_GAN_UPSAMPLE) != 0, pre = (d.flags & TTS_GAN_PRE_LRELU) != 0, vec = (cin & 3) == 0;
  const int hs = up ? h >> 1 : h;

  // this thread's share of the loads: pixel row ar of the tile, channels ak .. ak+3 of the step; weight row bk, columns bn .. bn+3
  const int ar = tid >> 2, ak = (tid & 3) * 4, bk = tid >> 4, bn = (tid & 15) * 4;
  const int am = m0 + ar;
  const bool arow = am < M;
  int an = 0, ay = 0, ax = 0;
  if (arow) {
    an = am / hw;
    const int r = am - an * hw;
    ay = r / h;
    ax = r - ay * h;
  }
  const int nsteps = cin_pad / GAN_KC, total = d.taps * nsteps;
  float4 ra, rb;
  auto load = [&](int it) {
    const int t = it / nsteps, c = (it - t * nsteps) * GAN_KC + ak;
    const int yy = ay + (d.taps == 9 ? t / 3 - 1 : 0), xx = ax + (d.taps == 9 ? t % 3 - 1 : 0);
    ra = make_float4(0.f, 0.f, 0.f, 0.f);
    if (arow && yy >= 0 && yy < h && xx >= 0 && xx < h && c < cin) {
      const int sy = up ? yy >> 1 : yy, sx = up ? xx >> 1 : xx;
      const float* p = d.x + ((static_cast<size_t>(an) * hs + sy) * hs + sx) * cin + c;
      if (vec) {  // cin and c multiples of 4: c + 3 < cin, 16-byte aligned
        ra = *reinterpret_cast<const float4*>(p);
      } else {
        ra.x = p[0];
        ra.y = c + 1 < cin ? p[1] : 0.f;
        ra.z = c + 2 < cin ? p[2] : 0.f;
        ra.w = c + 3 < cin ? p[3] : 0.f;
      }
      if (pre) {
        ra.x = lrelu(ra.x, d.pre_slope);
        ra.y = lrelu(ra.y, d.pre_slope);
        ra.z = lrelu(ra.z, d.pre_slope);
        ra.w = lrelu(ra.w, d.pre_slope);
      }
    }
    const int kb = t * cin_pad + (it - t * nsteps) * GAN_KC + bk;
    rb = *reinterpret_cast<const float4*>(d.w + static_cast<size_t>(kb) * cout_pad + n0 + bn);
  };

  const int msub = (wv & 1) * 32, nsub = (wv >> 1) * 32, li = lane & 31, lk = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  load(0);
  for (int it = 0; it < total; ++it) {
    __syncthreads();  // the previous step's operands have been read
    As[ak + 0][ar] = ra.x;
    As[ak + 1][ar] = ra.y;
    As[ak + 2][ar] = ra.z;
    As[ak + 3][ar] = ra.w;
    *reinterpret_cast<float4*>(&Bs[bk][bn]) = rb;
    __syncthreads();
    if (it + 1 < total) load(it + 1);
#pragma unroll
    for (int kk = 0; kk < GAN_KC; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + lk][msub + li], Bs[kk + lk][nsub + li], acc, 0, 0, 0);
  }

  // epilogue: lane holds column nsub + (lane & 31), rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the wave's quarter
  const int col = n0 + nsub + li;
  if (col >= d.cout) return;
  const float sc = d.scale ? d.scale[col] : 1.f, sh = d.shift ? d.shift[col] : 0.f;
  const bool res = (d.flags & TTS_GAN_RESIDUAL) != 0, res_up = (d.flags & TTS_GAN_RES_UPSAMPLE) != 0;
  const bool act = (d.flags & TTS_GAN_LRELU) != 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + msub + (r & 3) + 8 * (r >> 2) + 4 * lk;
    if (m >= M) continue;
    float v = acc[r] * sc + sh;
    if (res) {
      size_t ri = static_cast<size_t>(m);
      if (res_up) {
        const int n = m / hw, q = m - n * hw, y = q / h, x = q - y * h, hr = h >> 1;
        ri = (static_cast<size_t>(n) * hr + (y >> 1)) * hr + (x >> 1);
      }
      v = d.res[ri * d.cout + col] + d.res_ratio * v;
    }
    if (act) v = lrelu(v, d.slope);
    d.y[static_cast<size_t>(m) * d.cout + col] = v;
  }
}

static int gan_conv2d(const TtsGanConvDesc* d, hipStream_t stream) {
  TTS_CHECK_ARG(d != nullptr, "tts_gan_conv2d: null descriptor");
  TTS_CHECK_ARG(d->x && d->w && d->y, "tts_gan_conv2d: null x, w or y");
  TTS_CHECK_ARG(d->n >= 0 && d->h >= 1 && d->cin >= 1 && d->cout >= 1, "tts_gan_conv2d: bad shape n=%d h=%d cin=%d cout=%d", d->n,
                d->h, d->cin, d->cout);
  TTS_CHECK_ARG(d->taps == 9 || d->taps == 1, "tts_gan_conv2d: taps must be 9 (3x3) or 1 (1x1), got %d", d->taps);
  const int known = TTS_GAN_UPSAMPLE | TTS_GAN_PRE_LRELU | TTS_GAN_RESIDUAL | TTS_GAN_RES_UPSAMPLE | TTS_GAN_LRELU;
  TTS_CHECK_ARG((d->flags & ~known) == 0, "tts_gan_conv2d: unknown flags 0x%x", d->flags);
  TTS_CHECK_ARG(!(d->flags & (TTS_GAN_UPSAMPLE | TTS_GAN_RES_UPSAMPLE)) || (d->h & 1) == 0, "tts_gan_conv2d: an upsampled read needs an even h");
  TTS_CHECK_ARG(!(d->flags & TTS_GAN_RESIDUAL) || d->res, "tts_gan_conv2d: TTS_GAN_RESIDUAL without res");
  TTS_CHECK_ARG(!(d->flags & TTS_GAN_RES_UPSAMPLE) || (d->flags & TTS_GAN_RESIDUAL), "tts_gan_conv2d: TTS_GAN_RES_UPSAMPLE without TTS_GAN_RESIDUAL");
  TTS_CHECK_ARG((d->cin & 3) != 0 || (reinterpret_cast<uintptr_t>(d->x) & 15) == 0, "tts_gan_conv2d: x must be 16-byte aligned");
  TTS_CHECK_ARG((reinterpret_cast<uintptr_t>(d->w) & 15) == 0, "tts_gan_conv2d: w must be 16-byte aligned");
  const long long M = static_cast<long long>(d->n) * d->h * d->h;
  TTS_CHECK_ARG(M <= (1ll << 30), "tts_gan_conv2d: %lld pixels in one call, at most 2^30", M);
  TTS_CHECK_ARG(static_cast<long long>(d->taps) * d->cin <= (1 << 24) && d->cout <= (1 << 20), "tts_gan_conv2d: cin or cout too large");
  if (M == 0) return TTS_OK;
  const int cin_pad = (d->cin + GAN_KC - 1) / GAN_KC * GAN_KC, cout_pad = (d->cout + GAN_BN - 1) / GAN_BN * GAN_BN;
  const dim3 grid(static_cast<unsigned>((M + GAN_BM - 1) / GAN_BM), static_cast<unsigned>(cout_pad / GAN_BN));
  hipLaunchKernelGGL(gan_conv2d_kernel, grid, dim3(GAN_THREADS), 0, stream, *d, cin_pad, cout_pad, static_cast<int>(M));
  return launch_status("tts_gan_conv2d");
}

}  // namespace tts

extern "C" {
int tts_gan_conv2d(const TtsGanConvDesc* d, tts_stream_t stream) { return tts::gan_conv2d(d, reinterpret_cast<hipStream_t>(stream)); }
}
