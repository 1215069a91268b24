// Tube augmentation in front of the feature extractor, on the device: TubePreprocessor.preprocess_image
// (src/util/tube_augmentation.py:114-186) = tf.image.resize_images (bilinear, align_corners=False) -> edge pad ->
// img_size crop -> optional tf.contrib.image.rotate('BILINEAR') -> optional tf.reverse along x -> (v - 0.5) * 2.
// One gather kernel: the scaled image, the padded image and the un-rotated crop are never materialised.  Every
// output pixel clamps its coordinates into the scaled image (that IS the edge padding) and evaluates the four taps of
// TF 1.8's ResizeBilinear directly on the source frame; with rotation, each of the four taps of the rotation is such
// a crop pixel (or 0.0 outside the crop).  All arithmetic is float32 in the order include/hmmr_hip.h states, and this
// file is compiled with -ffp-contract=off: the NumPy oracle (tests/tube_oracle.py) performs the same IEEE operations.
// The per-frame integers, flip bytes and rotation rows come from the host mirror (util/tube_augmentation.py), where
// TF's float32 truncations are reproduced.  12 B written per output pixel; the reads hit cache.
#include "common.h"
#include "hmmr_hip.h"
#include "image_geom.h"

namespace {
using hmmr_img::tf_taps;

template <bool U8> struct src_elem;
template <> struct src_elem<true> { typedef unsigned char type; };
template <> struct src_elem<false> { typedef float type; };

// geom[f] = {newH, newW, x0, y0}: scaled image size and the scaled-image coordinates of crop pixel (0,0)
template <bool ROT, bool U8>
__global__ void tube_augment_kernel(const typename src_elem<U8>::type* __restrict__ images, const int4* __restrict__ geom,
                                    const unsigned char* __restrict__ flip, const float* __restrict__ rot,
                                    int n, int H, int W, int S, float* __restrict__ out) {
    // (float)((double)b / 255.0): the float32 the writers feed for a uint8 frame (image / 255.)
    __shared__ float lut[256];
    if (U8) {
        lut[threadIdx.x] = (float)((double)threadIdx.x / 255.0);
        __syncthreads();
    }
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * S * S) return;
    const int xo = (int)(i % S), y = (int)((i / S) % S), f = (int)(i / ((long long)S * S));
    const int4 g = geom[f];
    const int x = flip[f] ? S - 1 - xo : xo;                 // tf.reverse(image, [1]), applied after the rotation
    const typename src_elem<U8>::type* fr = images + (long long)f * H * W * 3;

    // crop pixel (cx, cy), three channels: the ResizeBilinear sample at the clamped scaled-image coordinates
    auto crop_px = [&](int cx, int cy, float (&v)[3]) {
        const int u = max(min(g.z + cx, g.y - 1), 0);        // clamp = the edge pad (max last: never negative)
        const int w = max(min(g.w + cy, g.x - 1), 0);
        int xl, xh, yl, yh; float xw, yw;
        tf_taps(u, W, g.y, xl, xh, xw);
        tf_taps(w, H, g.x, yl, yh, yw);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            auto px = [&](int yy, int xx) -> float {
                if (U8) return lut[(unsigned char)fr[((long long)yy * W + xx) * 3 + c]];
                return (float)fr[((long long)yy * W + xx) * 3 + c];
            };
            const float tl = px(yl, xl), tr = px(yl, xh), bl = px(yh, xl), br = px(yh, xh);
            const float top = tl + (tr - tl) * xw;
            const float bot = bl + (br - bl) * xw;
            v[c] = top + (bot - top) * yw;
        }
    };

    float v[3];
    if (ROT) {
        const float* a = rot + (long long)f * 6;             // output -> input: [cos, -sin, xoff, sin, cos, yoff]
        const float fx = a[0] * (float)x + a[1] * (float)y + a[2];
        const float fy = a[3] * (float)x + a[4] * (float)y + a[5];
        const float xf = floorf(fx), yf = floorf(fy);
        const float xc = xf + 1.f, yc = yf + 1.f;
        const float fS = (float)S;
        // a tap outside [0, S) reads 0.0 (tf.contrib.image: read_with_fill_value)
        auto tap = [&](float ty, float tx, float (&t)[3]) {
            if (ty >= 0.f && ty < fS && tx >= 0.f && tx < fS) crop_px((int)tx, (int)ty, t);
            else t[0] = t[1] = t[2] = 0.f;
        };
        float ff[3], fc[3], cf[3], cc[3];
        tap(yf, xf, ff); tap(yf, xc, fc); tap(yc, xf, cf); tap(yc, xc, cc);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float row_f = (xc - fx) * ff[c] + (fx - xf) * fc[c];
            const float row_c = (xc - fx) * cf[c] + (fx - xf) * cc[c];
            v[c] = (yc - fy) * row_f + (fy - yf) * row_c;
        }
    } else {
        crop_px(x, y, v);
    }
    float* o = out + i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (v[c] - 0.5f) * 2.0f;   // rescale_image, data_utils.py:370-378
}

template <bool ROT, bool U8>
void launch(const void* images, const int32_t* geom, const unsigned char* flip, const float* rot, int n, int h, int w, int S,
            float* out, hipStream_t stream) {
    const long long tot = (long long)n * S * S;
    hipLaunchKernelGGL((tube_augment_kernel<ROT, U8>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream,
                       (const typename src_elem<U8>::type*)images, (const int4*)geom, flip, rot, n, h, w, S, out);
}
}  // namespace

extern "C" int hmmr_tube_augment(const void* images, int images_are_u8, int n, int h, int w, const int32_t* geom,
                                 const unsigned char* flip, const float* rot, int S, float* out, void* stream) {
    HMMR_REQUIRE(images && geom && flip && out, "hmmr_tube_augment: null images, geom, flip or out");
    HMMR_REQUIRE(n > 0 && h > 0 && w > 0 && S > 0, "hmmr_tube_augment: n, h, w and S must be positive (n=%d h=%d w=%d S=%d)", n, h, w, S);
    HMMR_REQUIRE((long long)n * S * S <= 0x7fffffffll * 256, "hmmr_tube_augment: n * S * S = %lld output pixels exceed one launch",
                 (long long)n * S * S);
    const hipStream_t st = (hipStream_t)stream;
    if (rot) {
        if (images_are_u8) launch<true, true>(images, geom, flip, rot, n, h, w, S, out, st);
        else launch<true, false>(images, geom, flip, rot, n, h, w, S, out, st);
    } else {
        if (images_are_u8) launch<false, true>(images, geom, flip, rot, n, h, w, S, out, st);
        else launch<false, false>(images, geom, flip, rot, n, h, w, S, out, st);
    }
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}
