// quant.h -- a float source quantised inside the encoders (sprintz_mi355x_compress_batch_float / _float_dense): the one place the
// arithmetic is stated.  Element e of the source is in column d = e % ndims (chunk_len % ndims == 0); x is float32, float16 or bfloat16:
//   v = (float32) x                                  exact for the 16-bit formats
//   t = fl32(fl32(v - offset[d]) * inv_scale[d])     two IEEE float32 operations, never contracted
//   r = rint(t), ties to even -- or floor(t) with kQuantFloorBit
//   q = 0 where r is NaN, else clamp(r, LO, HI)      LO / HI = 0 / 2^W - 1, or -2^(W-1) / 2^(W-1) - 1 with kFloatSignedBit
// and the encoder takes q as a W-bit two's-complement element: the stream is the one the integer tensor q compresses to.
// The mode word is float rows' (geom.h): the format in its low two bits, kFloatSignedBit, and kQuantFloorBit next to it.  The format is
// wave-uniform, so a branch on it costs a scalar compare.
#pragma once

#include "sprintz_device.h"

namespace sprintz {

constexpr uint32_t kQuantFloorBit = 8;

// log2 of a source element's bytes
__device__ __forceinline__ uint32_t quant_src_shift(uint32_t mode) { return (mode & 3u) == kFloatF32 ? 2u : 1u; }

__device__ __forceinline__ float quant_f16_bits(uint32_t h) { return (float)__builtin_bit_cast(_Float16, (uint16_t)h); }
__device__ __forceinline__ float quant_bf16_bits(uint32_t h) { return __uint_as_float(h << 16); }
// the low 16 bits of h as a float16 (fmt == kFloatF16) or a bfloat16
__device__ __forceinline__ float quant_half_bits(uint32_t h, uint32_t fmt) { return fmt == kFloatF16 ? quant_f16_bits(h & 0xffffu) : quant_bf16_bits(h & 0xffffu); }

// element idx of a source of format fmt, as float32: one load of the element's own bytes
__device__ __forceinline__ float quant_load(const void* src, uint32_t fmt, uint64_t idx)
{
    if (fmt == kFloatF32) return ((const float*)src)[idx];
    return quant_half_bits(((const uint16_t*)src)[idx], fmt);
}

__device__ __forceinline__ float quant_inv_scale(const float* inv, uint32_t col) { return inv ? inv[col] : 1.0f; }
__device__ __forceinline__ float quant_offset(const float* off, uint32_t col) { return off ? off[col] : 0.0f; }

// v -> q, as the W-bit element (nothing above bit W)
template <int W>
__device__ __forceinline__ uint32_t quant_value(float v, float inv, float off, uint32_t mode)
{
#pragma clang fp contract(off)
    const float s = v - off;
    const float t = s * inv;
    const float r = (mode & kQuantFloorBit) ? __builtin_floorf(t) : __builtin_rintf(t);
    const float lo = (mode & kFloatSignedBit) ? -(float)(1 << (W - 1)) : 0.0f;
    const float hi = (mode & kFloatSignedBit) ? (float)((1 << (W - 1)) - 1) : (float)((1 << W) - 1);
    const float c = r < lo ? lo : (r > hi ? hi : r);          // (a NaN passes both comparisons)
    const int q = r != r ? 0 : (int)c;
    return (uint32_t)q & Elem<W>::MASK;
}

// One 16-byte piece of elements (NE = 8 of 16 bits, 16 of 8) from its raw source: NE float32 are raw[0 .. NE / 4), NE 16-bit floats
// raw[0 .. NE / 8).  inv / off: the scale and offset of the piece's elements, which the lane holds
template <int W>
__device__ __forceinline__ uint4 quant_piece(const uint4 (&raw)[32 / W], uint32_t mode, const float (&inv)[128 / W], const float (&off)[128 / W])
{
    constexpr int NE = 128 / W;
    const uint32_t fmt = mode & 3u;
    uint32_t q[NE];
    if (fmt == kFloatF32) {
#pragma unroll
        for (int j = 0; j < NE; j++) {
            const uint4& r = raw[j >> 2];
            const uint32_t b = (j & 3) == 0 ? r.x : (j & 3) == 1 ? r.y : (j & 3) == 2 ? r.z : r.w;
            q[j] = quant_value<W>(__uint_as_float(b), inv[j], off[j], mode);
        }
    } else {
#pragma unroll
        for (int j = 0; j < NE; j++) {
            const uint4& r = raw[j >> 3];
            const uint32_t b = ((j >> 1) & 3) == 0 ? r.x : ((j >> 1) & 3) == 1 ? r.y : ((j >> 1) & 3) == 2 ? r.z : r.w;
            q[j] = quant_value<W>(quant_half_bits(b >> (16 * (j & 1)), fmt), inv[j], off[j], mode);
        }
    }
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < NE; j++) {
        if constexpr (W == 16) w[j >> 1] |= q[j] << (16 * (j & 1));
        else w[j >> 2] |= q[j] << (8 * (j & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace sprintz
