// quic_crypto.h -- the cipher primitives of QUIC packet protection, restated
// from FIPS 197 (AES-128), NIST SP 800-38D (GHASH) and RFC 8439 (ChaCha20,
// Poly1305).  Nothing protocol-specific lives here; quic.hip composes them.
#pragma once
#include "kernels.h"

namespace hyobfs {
namespace quic {

HY_HD uint32_t rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

HY_HD uint32_t bswap32(uint32_t x) {
    return (x >> 24) | ((x >> 8) & 0xff00) | ((x << 8) & 0xff0000) | (x << 24);
}

// ------------------------------------------------------------------ AES-128 (FIPS 197), T-table in LDS
__constant__ uint8_t kSbox[256] = {
    0x63, 0x7c, 0x77, 0x7b, 0xf2, 0x6b, 0x6f, 0xc5, 0x30, 0x01, 0x67, 0x2b, 0xfe, 0xd7, 0xab, 0x76, 0xca, 0x82, 0xc9,
    0x7d, 0xfa, 0x59, 0x47, 0xf0, 0xad, 0xd4, 0xa2, 0xaf, 0x9c, 0xa4, 0x72, 0xc0, 0xb7, 0xfd, 0x93, 0x26, 0x36, 0x3f,
    0xf7, 0xcc, 0x34, 0xa5, 0xe5, 0xf1, 0x71, 0xd8, 0x31, 0x15, 0x04, 0xc7, 0x23, 0xc3, 0x18, 0x96, 0x05, 0x9a, 0x07,
    0x12, 0x80, 0xe2, 0xeb, 0x27, 0xb2, 0x75, 0x09, 0x83, 0x2c, 0x1a, 0x1b, 0x6e, 0x5a, 0xa0, 0x52, 0x3b, 0xd6, 0xb3,
    0x29, 0xe3, 0x2f, 0x84, 0x53, 0xd1, 0x00, 0xed, 0x20, 0xfc, 0xb1, 0x5b, 0x6a, 0xcb, 0xbe, 0x39, 0x4a, 0x4c, 0x58,
    0xcf, 0xd0, 0xef, 0xaa, 0xfb, 0x43, 0x4d, 0x33, 0x85, 0x45, 0xf9, 0x02, 0x7f, 0x50, 0x3c, 0x9f, 0xa8, 0x51, 0xa3,
    0x40, 0x8f, 0x92, 0x9d, 0x38, 0xf5, 0xbc, 0xb6, 0xda, 0x21, 0x10, 0xff, 0xf3, 0xd2, 0xcd, 0x0c, 0x13, 0xec, 0x5f,
    0x97, 0x44, 0x17, 0xc4, 0xa7, 0x7e, 0x3d, 0x64, 0x5d, 0x19, 0x73, 0x60, 0x81, 0x4f, 0xdc, 0x22, 0x2a, 0x90, 0x88,
    0x46, 0xee, 0xb8, 0x14, 0xde, 0x5e, 0x0b, 0xdb, 0xe0, 0x32, 0x3a, 0x0a, 0x49, 0x06, 0x24, 0x5c, 0xc2, 0xd3, 0xac,
    0x62, 0x91, 0x95, 0xe4, 0x79, 0xe7, 0xc8, 0x37, 0x6d, 0x8d, 0xd5, 0x4e, 0xa9, 0x6c, 0x56, 0xf4, 0xea, 0x65, 0x7a,
    0xae, 0x08, 0xba, 0x78, 0x25, 0x2e, 0x1c, 0xa6, 0xb4, 0xc6, 0xe8, 0xdd, 0x74, 0x1f, 0x4b, 0xbd, 0x8b, 0x8a, 0x70,
    0x3e, 0xb5, 0x66, 0x48, 0x03, 0xf6, 0x0e, 0x61, 0x35, 0x57, 0xb9, 0x86, 0xc1, 0x1d, 0x9e, 0xe1, 0xf8, 0x98, 0x11,
    0x69, 0xd9, 0x8e, 0x94, 0x9b, 0x1e, 0x87, 0xe9, 0xce, 0x55, 0x28, 0xdf, 0x8c, 0xa1, 0x89, 0x0d, 0xbf, 0xe6, 0x42,
    0x68, 0x41, 0x99, 0x2d, 0x0f, 0xb0, 0x54, 0xbb, 0x16};

// Te[x] = (2s, s, s, 3s) as little-endian bytes, s = S[x]; S[x] = (Te[x] >> 8) & 0xff.
__device__ __forceinline__ void aes_table_load(uint32_t* te, uint32_t lane) {
    for (uint32_t x = lane; x < 256; x += 64) {
        const uint32_t s = kSbox[x];
        const uint32_t s2 = ((s << 1) ^ ((s & 0x80) ? 0x1b : 0)) & 0xff;
        te[x] = s2 | s << 8 | s << 16 | (s2 ^ s) << 24;
    }
}

__device__ __forceinline__ uint32_t sub_word(const uint32_t* te, uint32_t w) {
    return ((te[w & 0xff] >> 8) & 0xff) | (te[(w >> 8) & 0xff] & 0xff00) | ((te[(w >> 16) & 0xff] << 8) & 0xff0000) |
           ((te[w >> 24] << 16) & 0xff000000u);
}

// round keys as little-endian column words, written to LDS as they are made
// (a 4-word window in registers); called by one lane
__device__ __forceinline__ void aes_expand_to(const uint32_t* te, const uint32_t k[4], uint32_t* dst) {
    uint32_t w0 = k[0], w1 = k[1], w2 = k[2], w3 = k[3];
    dst[0] = w0; dst[1] = w1; dst[2] = w2; dst[3] = w3;
    uint32_t rcon = 1;
#pragma unroll
    for (int r = 1; r <= 10; ++r) {
        w0 ^= sub_word(te, (w3 >> 8) | (w3 << 24)) ^ rcon;
        w1 ^= w0;
        w2 ^= w1;
        w3 ^= w2;
        rcon = ((rcon << 1) ^ ((rcon & 0x80) ? 0x1b : 0)) & 0xff;
        dst[4 * r] = w0; dst[4 * r + 1] = w1; dst[4 * r + 2] = w2; dst[4 * r + 3] = w3;
    }
}

__device__ __forceinline__ void aes_encrypt(const uint32_t* te, const uint32_t* rk, const uint32_t in[4],
                                            uint32_t out[4]) {
    uint32_t s0 = in[0] ^ rk[0], s1 = in[1] ^ rk[1], s2 = in[2] ^ rk[2], s3 = in[3] ^ rk[3];
#pragma unroll
    for (int r = 1; r < 10; ++r) {
        const uint32_t t0 = te[s0 & 0xff] ^ rotl(te[(s1 >> 8) & 0xff], 8) ^ rotl(te[(s2 >> 16) & 0xff], 16) ^
                            rotl(te[s3 >> 24], 24) ^ rk[4 * r];
        const uint32_t t1 = te[s1 & 0xff] ^ rotl(te[(s2 >> 8) & 0xff], 8) ^ rotl(te[(s3 >> 16) & 0xff], 16) ^
                            rotl(te[s0 >> 24], 24) ^ rk[4 * r + 1];
        const uint32_t t2 = te[s2 & 0xff] ^ rotl(te[(s3 >> 8) & 0xff], 8) ^ rotl(te[(s0 >> 16) & 0xff], 16) ^
                            rotl(te[s1 >> 24], 24) ^ rk[4 * r + 2];
        const uint32_t t3 = te[s3 & 0xff] ^ rotl(te[(s0 >> 8) & 0xff], 8) ^ rotl(te[(s1 >> 16) & 0xff], 16) ^
                            rotl(te[s2 >> 24], 24) ^ rk[4 * r + 3];
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
    auto sb = [&](uint32_t x) { return (te[x] >> 8) & 0xff; };
    out[0] = (sb(s0 & 0xff) | sb((s1 >> 8) & 0xff) << 8 | sb((s2 >> 16) & 0xff) << 16 | sb(s3 >> 24) << 24) ^ rk[40];
    out[1] = (sb(s1 & 0xff) | sb((s2 >> 8) & 0xff) << 8 | sb((s3 >> 16) & 0xff) << 16 | sb(s0 >> 24) << 24) ^ rk[41];
    out[2] = (sb(s2 & 0xff) | sb((s3 >> 8) & 0xff) << 8 | sb((s0 >> 16) & 0xff) << 16 | sb(s1 >> 24) << 24) ^ rk[42];
    out[3] = (sb(s3 & 0xff) | sb((s0 >> 8) & 0xff) << 8 | sb((s1 >> 16) & 0xff) << 16 | sb(s2 >> 24) << 24) ^ rk[43];
}

// ------------------------------------------------------------------ GF(2^128) (SP 800-38D 6.3)
// Block as a 128-bit big-endian integer (h = bytes 0..7, l = bytes 8..15);
// bit 0 of the field element is the MSB of byte 0.
struct G128 {
    uint64_t h, l;
};

// 16 block bytes as 4 little-endian words -> G128
HY_HD G128 g_from_le(const uint32_t w[4]) {
    return G128{(uint64_t)bswap32(w[0]) << 32 | bswap32(w[1]), (uint64_t)bswap32(w[2]) << 32 | bswap32(w[3])};
}

// times x: one right shift with the reduction x^128 = x^7 + x^2 + x + 1
HY_HD G128 mulx(G128 v) {
    const uint64_t lsb = 0 - (v.l & 1);
    return G128{(v.h >> 1) ^ (lsb & 0xE100000000000000ull), (v.l >> 1) | (v.h << 63)};
}

// P^2: squaring is linear over GF(2): spread the bits of the natural-order
// polynomial (bit i = x^i, the bit reversal of GCM's order), then fold the
// upper 128 bits with x^128 = x^7 + x^2 + x + 1
HY_HD uint64_t spread32(uint64_t x) {
    x = (x | x << 16) & 0x0000FFFF0000FFFFull;
    x = (x | x << 8) & 0x00FF00FF00FF00FFull;
    x = (x | x << 4) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | x << 2) & 0x3333333333333333ull;
    return (x | x << 1) & 0x5555555555555555ull;
}

HY_HD G128 gf_sqr(G128 v) {
    const uint64_t n0 = __builtin_bitreverse64(v.h), n1 = __builtin_bitreverse64(v.l);
    const uint64_t s0 = spread32(n0 & 0xffffffffu), s1 = spread32(n0 >> 32);
    const uint64_t s2 = spread32(n1 & 0xffffffffu), s3 = spread32(n1 >> 32);
    const uint64_t o = (s3 >> 63) ^ (s3 >> 62) ^ (s3 >> 57);   // degrees 128..134 of the shifted copies
    const uint64_t r0 = s0 ^ s2 ^ (s2 << 1) ^ (s2 << 2) ^ (s2 << 7) ^ o ^ (o << 1) ^ (o << 2) ^ (o << 7);
    const uint64_t r1 = s1 ^ s3 ^ (s3 << 1 | s2 >> 63) ^ (s3 << 2 | s2 >> 62) ^ (s3 << 7 | s2 >> 57);
    return G128{__builtin_bitreverse64(r0), __builtin_bitreverse64(r1)};
}

// Shoup's 4-bit tables (a wave-uniform multiplier P): tab[i] = P * i(x), nibble
// bit 3 = x^0 .. bit 0 = x^3 in GCM's reflected order; lanes 0..15 write one each.
__device__ __forceinline__ void shoup_build(G128* tab, G128 P, uint32_t lane) {
    if (lane < 16) {
        const G128 p1 = mulx(P), p2 = mulx(p1), p3 = mulx(p2);
        G128 e{0, 0};
        if (lane & 8) { e.h ^= P.h; e.l ^= P.l; }
        if (lane & 4) { e.h ^= p1.h; e.l ^= p1.l; }
        if (lane & 2) { e.h ^= p2.h; e.l ^= p2.l; }
        if (lane & 1) { e.h ^= p3.h; e.l ^= p3.l; }
        tab[lane] = e;
    }
}

// x * P through P's table: Horner over the 32 nibbles of x, last nibble first
__device__ __forceinline__ G128 shoup_mul(G128 x, const G128* tab) {
    G128 z{0, 0};
#pragma unroll 4
    for (int j = 31; j >= 0; --j) {
        if (j != 31) {
            // the 4 dropped bits times x^4: clmul(rem, 0x1C20) in the top 16 bits
            const uint32_t rem = (uint32_t)z.l & 0xf;
            const uint32_t red = ((rem & 1) * 0x1C20u) ^ ((rem & 2) * 0x1C20u) ^ ((rem & 4) * 0x1C20u) ^
                                 ((rem & 8) * 0x1C20u);
            z.l = (z.l >> 4) | (z.h << 60);
            z.h = (z.h >> 4) ^ ((uint64_t)red << 48);
        }
        const uint32_t nib = j >= 16 ? (uint32_t)(x.l >> (4 * (31 - j))) & 0xf : (uint32_t)(x.h >> (4 * (15 - j))) & 0xf;
        const G128 t = tab[nib];
        z.h ^= t.h;
        z.l ^= t.l;
    }
    return z;
}

// ------------------------------------------------------------------ ChaCha20 (RFC 8439 2.3)
HY_HD void chacha_qr(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
    a += b; d = rotl(d ^ a, 16);
    c += d; b = rotl(b ^ c, 12);
    a += b; d = rotl(d ^ a, 8);
    c += d; b = rotl(b ^ c, 7);
}

HY_HD void chacha20_block(const uint32_t key[8], uint32_t counter, const uint32_t nonce[3], uint32_t out[16]) {
    uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3],
                      key[4],      key[5],      key[6],      key[7],      counter, nonce[0], nonce[1], nonce[2]};
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = s[i];
    for (int r = 0; r < 10; ++r) {
        chacha_qr(x[0], x[4], x[8], x[12]);
        chacha_qr(x[1], x[5], x[9], x[13]);
        chacha_qr(x[2], x[6], x[10], x[14]);
        chacha_qr(x[3], x[7], x[11], x[15]);
        chacha_qr(x[0], x[5], x[10], x[15]);
        chacha_qr(x[1], x[6], x[11], x[12]);
        chacha_qr(x[2], x[7], x[8], x[13]);
        chacha_qr(x[3], x[4], x[9], x[14]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) out[i] = x[i] + s[i];
}

// ------------------------------------------------------------------ Poly1305 (RFC 8439 2.5), 26-bit limbs
struct P130 {
    uint32_t v[5];
};

HY_HD P130 p_mul(const P130& a, const P130& r) {
    const uint64_t r0 = r.v[0], r1 = r.v[1], r2 = r.v[2], r3 = r.v[3], r4 = r.v[4];
    const uint64_t s1 = r1 * 5, s2 = r2 * 5, s3 = r3 * 5, s4 = r4 * 5;
    const uint64_t a0 = a.v[0], a1 = a.v[1], a2 = a.v[2], a3 = a.v[3], a4 = a.v[4];
    uint64_t d0 = a0 * r0 + a1 * s4 + a2 * s3 + a3 * s2 + a4 * s1;
    uint64_t d1 = a0 * r1 + a1 * r0 + a2 * s4 + a3 * s3 + a4 * s2;
    uint64_t d2 = a0 * r2 + a1 * r1 + a2 * r0 + a3 * s4 + a4 * s3;
    uint64_t d3 = a0 * r3 + a1 * r2 + a2 * r1 + a3 * r0 + a4 * s4;
    uint64_t d4 = a0 * r4 + a1 * r3 + a2 * r2 + a3 * r1 + a4 * r0;
    P130 o;
    uint64_t c = d0 >> 26; o.v[0] = (uint32_t)d0 & 0x3ffffff;
    d1 += c; c = d1 >> 26; o.v[1] = (uint32_t)d1 & 0x3ffffff;
    d2 += c; c = d2 >> 26; o.v[2] = (uint32_t)d2 & 0x3ffffff;
    d3 += c; c = d3 >> 26; o.v[3] = (uint32_t)d3 & 0x3ffffff;
    d4 += c; c = d4 >> 26; o.v[4] = (uint32_t)d4 & 0x3ffffff;
    uint64_t t = (uint64_t)o.v[0] + c * 5;
    o.v[0] = (uint32_t)t & 0x3ffffff;
    o.v[1] += (uint32_t)(t >> 26);
    return o;
}

// 16 little-endian bytes as 4 LE words, plus 2^128 when hibit
HY_HD P130 p_from_block(const uint32_t w[4], uint32_t hibit) {
    P130 o;
    o.v[0] = w[0] & 0x3ffffff;
    o.v[1] = ((w[0] >> 26) | (w[1] << 6)) & 0x3ffffff;
    o.v[2] = ((w[1] >> 20) | (w[2] << 12)) & 0x3ffffff;
    o.v[3] = ((w[2] >> 14) | (w[3] << 18)) & 0x3ffffff;
    o.v[4] = (w[3] >> 8) | (hibit << 24);
    return o;
}

}  // namespace quic
}  // namespace hyobfs
