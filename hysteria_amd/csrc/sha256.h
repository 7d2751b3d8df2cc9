// sha256.h -- SHA-256 (FIPS 180-4) and HMAC-SHA-256 (RFC 2104) for host and
// device code: the realm punch mask (realm.hip) and the QUIC Initial key
// schedule (quic.hip) share this one compression function.
#pragma once
#include "kernels.h"

namespace hyobfs {

// 4 bytes <-> one big-endian word
HY_HD uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
HY_HD void put_be32(uint8_t* p, uint32_t x) {
    p[0] = (uint8_t)(x >> 24); p[1] = (uint8_t)(x >> 16); p[2] = (uint8_t)(x >> 8); p[3] = (uint8_t)x;
}

HY_HD uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// one block (16 big-endian words) into the chaining state; rolling 16-word schedule
HY_HD void sha256_compress(uint32_t st[8], const uint32_t blk[16]) {
    const uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
        0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
        0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
        0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
        0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
        0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
        0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
        0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = blk[i];
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        if (i >= 16) {
            const uint32_t x = w[(i - 15) & 15], y = w[(i - 2) & 15];
            w[i & 15] += (rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3)) + w[(i - 7) & 15] + (rotr(y, 17) ^ rotr(y, 19) ^ (y >> 10));
        }
        const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i & 15];
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

HY_HD void sha256_init(uint32_t st[8]) {
    st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
    st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}

// HMAC-SHA-256 with a key of at most 64 bytes, as the two chaining states
// after the ipad / opad blocks (RFC 2104).
struct HmacKey {
    uint32_t in[8], out[8];
};

// key: big-endian words of the key zero-padded to 64 bytes
HY_HD void hmac_key(HmacKey& k, const uint32_t key[16]) {
    uint32_t b[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) b[i] = key[i] ^ 0x36363636u;
    sha256_init(k.in);
    sha256_compress(k.in, b);
#pragma unroll
    for (int i = 0; i < 16; ++i) b[i] = key[i] ^ 0x5c5c5c5cu;
    sha256_init(k.out);
    sha256_compress(k.out, b);
}

// a 32-byte key given as 8 big-endian words
HY_HD void hmac_key32(HmacKey& k, const uint32_t key[8]) {
    const uint32_t b[16] = {key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7]};   // zero-padded
    hmac_key(k, b);
}

// outer hash over the inner digest
HY_HD void hmac_finish(const HmacKey& k, const uint32_t inner[8], uint32_t mac[8]) {
    const uint32_t b[16] = {inner[0], inner[1], inner[2], inner[3], inner[4], inner[5], inner[6], inner[7],
                            0x80000000u, 0, 0, 0, 0, 0, 0, (64 + 32) * 8};   // padded; the opad block counts
#pragma unroll
    for (int i = 0; i < 8; ++i) mac[i] = k.out[i];
    sha256_compress(mac, b);
}

// HMAC of a message that fits one padded block (blk already padded, with the
// bit length counting the 64-byte ipad block).
HY_HD void hmac_block(const HmacKey& k, const uint32_t blk[16], uint32_t mac[8]) {
    uint32_t inner[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) inner[i] = k.in[i];
    sha256_compress(inner, blk);
    hmac_finish(k, inner, mac);
}

// HMAC of msg[0, len): the message is padded as it streams through, a block
// at a time (0x80, zeros, the bit length counting the ipad block).
__host__ __device__ inline void hmac_bytes(const HmacKey& k, const uint8_t* msg, uint32_t len, uint32_t mac[8]) {
    uint32_t st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = k.in[i];
    const uint32_t nb = (len + 9 + 63) / 64;
    for (uint32_t b = 0; b < nb; ++b) {
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            uint32_t x = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const uint32_t q = 64 * b + 4 * j + t;
                const uint32_t c = q < len ? msg[q] : (q == len ? 0x80u : 0u);
                x |= c << (24 - 8 * t);
            }
            w[j] = x;
        }
        if (b == nb - 1) w[15] = (64 + len) * 8;
        sha256_compress(st, w);
    }
    hmac_finish(k, st, mac);
}

}  // namespace hyobfs
