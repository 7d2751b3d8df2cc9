// quic.hip -- QUIC Initial unprotection for the sniffer (include/hyobfs_quic.h).
//
// Reference: apernet/hysteria extras/sniff/internal/quic (header.go, payload.go,
// packet_protector.go, quic.go).  The ciphers are Go's crypto/aes + cipher.GCM
// and golang.org/x/crypto chacha20 / chacha20poly1305 / hkdf, restated from
// FIPS 197, NIST SP 800-38D, RFC 8439, RFC 5869 and FIPS 180-4.
//
// Two kernels:
//   quic_prep_kernel   one LANE per packet: ParseInitialHeader, the version /
//                      length checks of ReadCryptoPayload, and the client
//                      Initial key schedule (HKDF-SHA-256: ~16 compressions)
//                      -> a 96-byte job record per packet in the workspace.
//   quic_open_kernel   one WAVE (a 64-thread workgroup) per packet: header
//                      protection (one AES / ChaCha20 block, computed by every
//                      lane), packet-number decode, AEAD verify (GHASH or
//                      Poly1305 evaluated as a polynomial split over the 64
//                      lanes: lane l takes blocks m-1-l-64t, Horner in H^64 /
//                      r^64, then one multiply by H^(l+1) / r^(l+1) and a
//                      cross-lane reduction), then decrypt in place (a CTR /
//                      ChaCha20 block per lane per step); for ReadCryptoPayload
//                      also the CRYPTO-frame walk (wave-uniform, padding runs
//                      skipped 64 bytes per ballot) and the assembly.
// The path is compute-bound, low volume (the first packets of a connection):
// correctness and per-packet latency matter more than HBM rate here.
// Built from sha256.h (SHA-256 / HMAC, shared with realm.hip) and quic_crypto.h
// (AES-128, GF(2^128), ChaCha20, Poly1305).
#include "kernels.h"
#include "../../include/hyobfs_quic.h"
#include "quic_crypto.h"
#include "sha256.h"

#include <cstring>
#include <vector>

namespace hyobfs {
namespace quic {

// ------------------------------------------------------------------ header parse (header.go:24-89)
// quicvarint.Read: 1/2/4/8-byte big-endian with the length in the top 2 bits
HY_HD bool read_varint(const uint8_t* p, uint64_t len, uint64_t& i, uint64_t& v) {
    if (i >= len) return false;
    const uint32_t n = 1u << (p[i] >> 6);
    if (len - i < n) return false;
    v = p[i] & 0x3f;
    for (uint32_t k = 1; k < n; ++k) v = (v << 8) | p[i + k];
    i += n;
    return true;
}

// fills h (only meaningful when the status is HYOBFS_OK) and returns the status
HY_HD int parse_initial_header(const uint8_t* p, uint64_t len, hyobfs_quic_header& h) {
    h = hyobfs_quic_header{};
    const int eof = HYOBFS_QUIC_ERR_EOF;
    if (len < 5) return eof;   // type byte + 4-byte version (ReadByte / io.ReadFull)
    h.type = p[0];
    h.version = be32(p + 1);
    if (h.version != 0 && (h.type & 0x40) == 0) return HYOBFS_QUIC_ERR_NOT_QUIC;
    uint64_t i = 5;
    // a connection ID that runs past the end is io.EOF, or (none of it
    // present) makes the next read fail with io.EOF: EOF either way
    if (i >= len) return eof;
    h.dcid_len = p[i++];
    if (len - i < h.dcid_len) return eof;
    h.dcid_off = (uint32_t)i;
    i += h.dcid_len;
    if (i >= len) return eof;
    h.scid_len = p[i++];
    if (len - i < h.scid_len) return eof;
    h.scid_off = (uint32_t)i;
    i += h.scid_len;
    const uint32_t initial_type = h.version == HYOBFS_QUIC_V2 ? 1u : 0u;
    if (((h.type >> 4) & 3u) == initial_type) {
        uint64_t tl;
        if (!read_varint(p, len, i, tl)) return eof;
        if (tl > len - i) return eof;
        h.token_off = (uint32_t)i;
        h.token_len = (uint32_t)tl;
        i += tl;
    }
    if (!read_varint(p, len, i, h.length)) return eof;
    h.offset = (int64_t)i;
    return HYOBFS_OK;
}

// decodePacketNumber (packet_protector.go:161-174), with Go's wrapping int64
HY_HD int64_t decode_packet_number(int64_t largest, int64_t truncated, uint32_t nbytes) {
    const int64_t expected = (int64_t)((uint64_t)largest + 1);
    const int64_t win = (int64_t)1 << (nbytes * 8);
    const int64_t hwin = win / 2;
    const int64_t mask = win - 1;
    const int64_t candidate = (expected & ~mask) | truncated;
    if (candidate <= (int64_t)((uint64_t)expected - (uint64_t)hwin) && candidate < ((int64_t)1 << 62) - win)
        return (int64_t)((uint64_t)candidate + (uint64_t)win);
    if (candidate > (int64_t)((uint64_t)expected + (uint64_t)hwin) && candidate >= win)
        return candidate - win;
    return candidate;
}

// One HKDF-Expand-Label message block: info(L, "tls13 "+label, "") || 0x01,
// padded, bit length counting the ipad block (packet_protector.go:177-193).
inline void label_block(const char* label, uint32_t L, uint32_t blk[16]) {
    const size_t ll = std::strlen(label);
    uint8_t b[64] = {(uint8_t)(L >> 8), (uint8_t)L, (uint8_t)(6 + ll), 't', 'l', 's', '1', '3', ' '};
    std::memcpy(b + 9, label, ll);
    size_t i = 9 + ll;
    b[i++] = 0;   // empty context
    b[i++] = 1;   // T(1) counter
    const uint32_t bits = (uint32_t)(64 + i) * 8;
    b[i] = 0x80;
    b[62] = (uint8_t)(bits >> 8);
    b[63] = (uint8_t)bits;
    for (int k = 0; k < 16; ++k) blk[k] = be32(b + 4 * k);
}

const uint8_t kSaltOld[20] = {0xaf, 0xbf, 0xec, 0x28, 0x99, 0x93, 0xd2, 0x4c, 0x9e, 0x97,
                              0x86, 0xf1, 0x9c, 0x61, 0x11, 0xe0, 0x43, 0x90, 0xa8, 0x99};
const uint8_t kSaltV1[20] = {0x38, 0x76, 0x2c, 0xf7, 0xf5, 0x59, 0x34, 0xb3, 0x4d, 0x17,
                             0x9a, 0xe6, 0xa4, 0xc8, 0x0c, 0xad, 0xcc, 0xbb, 0x7f, 0x0a};
const uint8_t kSaltV2[20] = {0x0d, 0xed, 0xe3, 0xde, 0xf7, 0x00, 0xa6, 0xdb, 0x81, 0x93,
                             0x81, 0xbe, 0x6e, 0x26, 0x9d, 0xcb, 0xf9, 0xbd, 0x2e, 0xd9};

// getSalt (quic.go:28-36)
inline const uint8_t* get_salt(uint32_t v) {
    return v == HYOBFS_QUIC_V1 ? kSaltV1 : v == HYOBFS_QUIC_V2 ? kSaltV2 : kSaltOld;
}

inline void key_words(const uint8_t* key, size_t n, uint32_t w[16]) {
    uint8_t b[64] = {};
    std::memcpy(b, key, n);
    for (int k = 0; k < 16; ++k) w[k] = be32(b + 4 * k);
}

// n bytes (a multiple of 4) of big-endian words
HY_HD void words_to_bytes(const uint32_t* w, uint8_t* out, uint32_t n) {
    for (uint32_t i = 0; i < n / 4; ++i) put_be32(out + 4 * i, w[i]);
}

// host HMAC over byte strings (key <= 64 bytes)
inline void hmac_host(const uint8_t* key, size_t kl, const uint8_t* msg, size_t ml, uint8_t out[32]) {
    uint32_t kw[16], mac[8];
    key_words(key, kl, kw);
    HmacKey k;
    hmac_key(k, kw);
    hmac_bytes(k, msg, (uint32_t)ml, mac);
    words_to_bytes(mac, out, 32);
}

// Everything the prep kernel needs that depends only on constants: the
// HMAC states of the two Initial salts and the HKDF-Expand-Label blocks.
struct PrepConsts {
    HmacKey salt[2];         // V1, V2
    uint32_t client_in[16];  // "client in", 32
    uint32_t key[2][16];     // "quic key" / "quicv2 key", 16
    uint32_t iv[2][16];      // "quic iv" / "quicv2 iv", 12
    uint32_t hp[2][16];      // "quic hp" / "quicv2 hp", 16
};

inline PrepConsts make_prep_consts() {
    PrepConsts c{};
    uint32_t w[16];
    key_words(kSaltV1, 20, w);
    hmac_key(c.salt[0], w);
    key_words(kSaltV2, 20, w);
    hmac_key(c.salt[1], w);
    label_block("client in", 32, c.client_in);
    label_block("quic key", 16, c.key[0]);
    label_block("quicv2 key", 16, c.key[1]);
    label_block("quic iv", 12, c.iv[0]);
    label_block("quicv2 iv", 12, c.iv[1]);
    label_block("quic hp", 16, c.hp[0]);
    label_block("quicv2 hp", 16, c.hp[1]);
    return c;
}

// per-packet record written by the prep kernel
struct Job {
    hyobfs_quic_key key;
    int64_t pn_offset;
    uint32_t len;    // offset + Length: the slice UnProtect sees
    int32_t status;
};
static_assert(sizeof(Job) == 96, "job record layout");
static_assert(sizeof(hyobfs_quic_key) == 80, "hyobfs_quic_key layout");
static_assert(sizeof(hyobfs_quic_result) == 24, "hyobfs_quic_result layout");

// ------------------------------------------------------------------ device byte access
__device__ __forceinline__ uint32_t le_word(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// bytes [pos, pos+16) of [0, n) as 4 LE words, zero past n
__device__ __forceinline__ void load_block(const uint8_t* p, uint64_t pos, uint64_t n, uint32_t w[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t x = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint64_t q = pos + 4 * k + b;
            x |= (q < n ? (uint32_t)p[q] : 0u) << (8 * b);
        }
        w[k] = x;
    }
}

__device__ __forceinline__ void store_xor(uint8_t* p, uint64_t pos, uint64_t n, const uint32_t* ct, const uint32_t* ks,
                                          int words) {
    for (int k = 0; k < words; ++k) {
        const uint32_t x = ct[k] ^ ks[k];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint64_t q = pos + 4 * k + b;
            if (q < n) p[q] = (uint8_t)(x >> (8 * b));
        }
    }
}

// ------------------------------------------------------------------ prep kernel
__global__ __launch_bounds__(256) void quic_prep_kernel(const uint8_t* packets, const uint64_t* off,
                                                        const uint32_t* len, uint64_t n, Job* jobs,
                                                        PrepConsts c) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* p = packets + off[i];
    const uint32_t L = len[i];
    Job j{};
    j.key.suite = HYOBFS_QUIC_TLS_AES_128_GCM_SHA256;
    // ReadCryptoPayload's checks (payload.go:22-46)
    hyobfs_quic_header h;
    int st = parse_initial_header(p, L, h);
    if (st == HYOBFS_OK && h.version != HYOBFS_QUIC_V1 && h.version != HYOBFS_QUIC_V2) st = HYOBFS_QUIC_ERR_VERSION;
    if (st == HYOBFS_OK && (h.offset == 0 || h.length == 0)) st = HYOBFS_QUIC_ERR_INVALID;
    if (st == HYOBFS_OK && (uint64_t)L - (uint64_t)h.offset < h.length) st = HYOBFS_QUIC_ERR_SHORT;
    if (st == HYOBFS_OK) {
        const int v = h.version == HYOBFS_QUIC_V2;
        uint32_t secret[8], mac[8];
        hmac_bytes(c.salt[v], p + h.dcid_off, h.dcid_len, secret);   // HKDF-Extract
        HmacKey k;
        hmac_key32(k, secret);
        hmac_block(k, c.client_in, secret);                    // "client in"
        hmac_key32(k, secret);
        hmac_block(k, c.key[v], mac);
        words_to_bytes(mac, j.key.key, 16);
        hmac_block(k, c.iv[v], mac);
        words_to_bytes(mac, j.key.iv, 12);
        hmac_block(k, c.hp[v], mac);
        words_to_bytes(mac, j.key.hp, 16);
        j.pn_offset = h.offset;
        j.len = (uint32_t)((uint64_t)h.offset + h.length);
    }
    j.status = st;
    jobs[i] = j;
}

// ------------------------------------------------------------------ open kernel
struct Frame {
    uint64_t off;
    uint32_t len;
    uint32_t pos;
};

struct OpenArgs {
    uint8_t* packets;
    const uint64_t* off;
    const uint32_t* len;
    uint64_t n;
    const hyobfs_quic_key* keys;
    uint32_t key_stride;
    const int64_t* pn_offset;
    const int64_t* pn_max;
    const Job* jobs;
    hyobfs_quic_result* res;
    uint8_t* out;
    const uint64_t* out_off;
    const uint32_t* out_cap;
};

// wave-uniform byte reader over [0, n): each lane holds one byte of a 64-byte window
struct Window {
    const uint8_t* p;
    uint64_t n, base;
    uint32_t mine;
    __device__ void fill(uint64_t at, uint32_t lane) {
        base = at;
        mine = at + lane < n ? p[at + lane] : 0u;
    }
    __device__ uint32_t get(uint64_t i, uint32_t lane) {
        if (i < base || i >= base + 64) fill(i, lane);
        return (uint32_t)__shfl((int)mine, (int)(i - base), 64) & 0xff;
    }
    __device__ bool varint(uint64_t& i, uint64_t& v, uint32_t lane) {
        if (i >= n) return false;
        const uint32_t b0 = get(i, lane);
        const uint32_t k = 1u << (b0 >> 6);
        if (n - i < k) return false;
        v = b0 & 0x3f;
        for (uint32_t t = 1; t < k; ++t) v = (v << 8) | get(i + t, lane);
        i += k;
        return true;
    }
};

// ---- the stages of the open kernel, in the order of UnProtect (packet_protector.go:46-79)
// and ReadCryptoPayload (payload.go:21-148).  All are inlined into the one kernel; the
// __shared__ arrays they work on are the kernel's.  Every branch around a barrier is
// packet-uniform, so all 64 lanes reach it.

// What UnProtect is called with: the prep kernel's job (ReadCryptoPayload) or the
// caller's arrays.  Returns the packet's status so far.
template <bool CRYPTO>
__device__ __forceinline__ int load_job(const OpenArgs& a, uint64_t pk, hyobfs_quic_key& key, int64_t& pn_off,
                                        int64_t& pn_max, uint64_t& L) {
    if (CRYPTO) {
        const Job& j = a.jobs[pk];
        key = j.key;
        pn_off = j.pn_offset;
        pn_max = 2;   // payload.go:47
        L = j.len;
        return j.status;
    }
    key = a.keys[pk * a.key_stride];
    pn_off = a.pn_offset[pk];
    pn_max = a.pn_max ? a.pn_max[pk] : 0;
    L = a.len[pk];
    return HYOBFS_OK;
}

// mask = headerProtection(sample), the 16-byte sample at pnOffset + 4
// (packet_protector.go:51-56): its first 5 bytes as two words.  AES: lane 0
// expands the round keys of hp and of the AEAD key into LDS on the way.
__device__ __forceinline__ void header_mask(bool aes, const uint32_t* te, uint32_t* hrkl, uint32_t* rkl,
                                            const uint32_t hpw[8], const uint32_t kw[8], const uint8_t* p,
                                            int64_t pn_off, uint64_t L, uint32_t lane, uint32_t& mw0, uint32_t& mw1) {
    uint32_t sample[4];
    load_block(p, (uint64_t)pn_off + 4, L, sample);
    if (aes) {
        uint32_t m[4];
        if (lane == 0) {
            aes_expand_to(te, hpw, hrkl);
            aes_expand_to(te, kw, rkl);
        }
        __syncthreads();
        aes_encrypt(te, hrkl, sample, m);
        mw0 = m[0];
        mw1 = m[1];
    } else {
        uint32_t ks[16];
        chacha20_block(hpw, sample[0], sample + 1, ks);
        mw0 = ks[0];
        mw1 = ks[1];
    }
}

// The header with its protection removed (packet_protector.go:57-72), kept in
// registers: the packet itself is rewritten only after the AEAD has read it.
struct Unmasked {
    uint32_t b0, first, pn_len, pmask;   // byte 0 as received / unmasked; pmask = mask[1..4]
    int64_t pn_off, pn;
    uint64_t hdr_len;
};

__device__ __forceinline__ Unmasked unmask_header(const uint8_t* p, int64_t pn_off, int64_t pn_max, uint32_t mw0,
                                                  uint32_t mw1, const uint32_t ivw[3], uint32_t nonce[3]) {
    Unmasked u;
    u.pn_off = pn_off;
    u.b0 = p[0];
    const bool long_hdr = (u.b0 & 0x80) != 0;
    u.first = u.b0 ^ (mw0 & (long_hdr ? 0x0fu : 0x1fu));
    u.pn_len = (u.first & 3) + 1;
    u.pmask = (mw0 >> 8) | (mw1 << 24);
    int64_t trunc = 0;
    for (uint32_t k = 0; k < u.pn_len; ++k)
        trunc = (trunc << 8) | ((p[pn_off + k] ^ (u.pmask >> (8 * k))) & 0xff);
    u.pn = decode_packet_number(pn_max, trunc, u.pn_len);
    u.hdr_len = (uint64_t)pn_off + u.pn_len;
    // nonce = iv ^ (0^32 || BE64(pn))  (packet_protector.go:93-100)
    nonce[0] = ivw[0];
    nonce[1] = ivw[1] ^ bswap32((uint32_t)((uint64_t)u.pn >> 32));
    nonce[2] = ivw[2] ^ bswap32((uint32_t)(uint64_t)u.pn);
    return u;
}

// What the AEAD authenticates, as a stream of m 16-byte blocks (4 LE words
// each): the AAD, the ciphertext, the length block.
struct AeadInput {
    const uint8_t* p;    // the packet: AAD = its unmasked header
    const uint8_t* ct;
    Unmasked u;
    uint64_t ct_len, aad_blocks, ct_blocks, m;

    // AAD = the unmasked header: substitute the unmasked bytes on the fly
    __device__ __forceinline__ void aad_block(uint64_t pos, uint32_t w[4]) const {
        load_block(p, pos, u.hdr_len, w);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint64_t q = pos + k;
            uint32_t fix = 0;
            if (q == 0) fix = (u.b0 ^ u.first) & 0xff;
            else if (q >= (uint64_t)u.pn_off && q < u.hdr_len) fix = (u.pmask >> (8 * (q - u.pn_off))) & 0xff;
            w[k / 4] ^= fix << (8 * (k % 4));
        }
    }
    __device__ __forceinline__ void block(uint64_t s, uint32_t w[4], bool le_lengths) const {
        if (s < aad_blocks) {
            aad_block(16 * s, w);
        } else if (s < aad_blocks + ct_blocks) {
            load_block(ct, 16 * (s - aad_blocks), ct_len, w);
        } else if (le_lengths) {   // Poly1305: LE64(aad) || LE64(ct)
            w[0] = (uint32_t)u.hdr_len; w[1] = (uint32_t)(u.hdr_len >> 32);
            w[2] = (uint32_t)ct_len; w[3] = (uint32_t)(ct_len >> 32);
        } else {                   // GHASH: BE64(aad bits) || BE64(ct bits), as LE words of those bytes
            const uint64_t ab = u.hdr_len * 8, cb = ct_len * 8;
            w[0] = bswap32((uint32_t)(ab >> 32)); w[1] = bswap32((uint32_t)ab);
            w[2] = bswap32((uint32_t)(cb >> 32)); w[3] = bswap32((uint32_t)cb);
        }
    }
};

// AES-128-GCM's tag check (SP 800-38D 7.2); nt = the blocks this lane takes
__device__ __forceinline__ bool gcm_tag_ok(const uint32_t* te, const uint32_t* rk, G128 (*gtab)[16],
                                           const uint32_t nonce[3], const uint32_t tagw[4], const AeadInput& in,
                                           uint64_t nt, uint32_t lane) {
    const uint64_t m = in.m;
    // H = E(K, 0) and Shoup tables of H^(2^k), k = 0..6
    const uint32_t zero[4] = {0, 0, 0, 0};
    uint32_t hw[4];
    aes_encrypt(te, rk, zero, hw);
    G128 P = g_from_le(hw);
    shoup_build(gtab[0], P, lane);
    for (int k = 1; k < 7; ++k) {
        P = gf_sqr(P);
        shoup_build(gtab[k], P, lane);
    }
    __syncthreads();
    // lane l: acc_l = sum_t X_{m-1-l-64t} H^(64t), Horner in the uniform H^64
    G128 acc{0, 0};
    for (uint64_t t = nt; t-- > 0;) {
        uint32_t w[4];
        in.block(m - 1 - lane - 64 * t, w, false);
        const G128 x = g_from_le(w);
        if (t + 1 != nt) acc = shoup_mul(acc, gtab[6]);
        acc.h ^= x.h;
        acc.l ^= x.l;
    }
    // lane tree: sum_l acc_l H^l, one multiply by the uniform H^(2^k) per level;
    // then times H, so block s carries H^(m-s)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int src = (int)((lane + (1u << k)) & 63);
        G128 b{__shfl(acc.h, src, 64), __shfl(acc.l, src, 64)};
        b = shoup_mul(b, gtab[k]);
        acc.h ^= b.h;
        acc.l ^= b.l;
    }
    acc = G128{__shfl(acc.h, 0, 64), __shfl(acc.l, 0, 64)};
    acc = shoup_mul(acc, gtab[0]);
    // tag = E(K, J0) ^ S
    const uint32_t j0[4] = {nonce[0], nonce[1], nonce[2], 0x01000000u};
    uint32_t ej[4];
    aes_encrypt(te, rk, j0, ej);
    const G128 ejg = g_from_le(ej);
    const G128 tg = g_from_le(tagw);
    return ((acc.h ^ ejg.h) == tg.h) && ((acc.l ^ ejg.l) == tg.l);
}

// ChaCha20-Poly1305's tag check (RFC 8439 2.8)
__device__ __forceinline__ bool poly1305_tag_ok(const uint32_t kw[8], const uint32_t nonce[3], const uint32_t tagw[4],
                                                const AeadInput& in, uint64_t nt, uint32_t lane) {
    const uint64_t m = in.m;
    // one-time key = ChaCha20(K, 0, nonce)[0:32] (RFC 8439 2.6)
    uint32_t otk[16];
    chacha20_block(kw, 0, nonce, otk);
    const uint32_t rw[4] = {otk[0] & 0x0fffffffu, otk[1] & 0x0ffffffcu, otk[2] & 0x0ffffffcu,
                            otk[3] & 0x0ffffffcu};
    const P130 R = p_from_block(rw, 0);
    P130 rp[7];
    rp[0] = R;
#pragma unroll
    for (int k = 1; k < 7; ++k) rp[k] = p_mul(rp[k - 1], rp[k - 1]);   // r^(2^k)
    P130 acc{{0, 0, 0, 0, 0}};
    for (uint64_t t = nt; t-- > 0;) {
        uint32_t w[4];
        in.block(m - 1 - lane - 64 * t, w, true);
        const P130 x = p_from_block(w, 1);
        acc = p_mul(acc, rp[6]);
#pragma unroll
        for (int k = 0; k < 5; ++k) acc.v[k] += x.v[k];
    }
    P130 pw{{1, 0, 0, 0, 0}};
    const uint32_t e = lane + 1;
#pragma unroll
    for (int k = 0; k < 7; ++k)
        if ((e >> k) & 1) pw = p_mul(pw, rp[k]);
    acc = nt ? p_mul(acc, pw) : P130{{0, 0, 0, 0, 0}};
    // sum over lanes (limbs < 2^27 each: the 64-lane sum fits 33 bits)
    uint64_t sum[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        uint64_t v = acc.v[k];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
        sum[k] = v;
    }
    // full reduction mod 2^130 - 5
    uint64_t c = 0;
    for (int pass = 0; pass < 3; ++pass) {   // limbs < 2^26, h < 2^130
        for (int k = 0; k < 5; ++k) {
            sum[k] += c;
            c = sum[k] >> 26;
            sum[k] &= 0x3ffffff;
        }
        sum[0] += c * 5;
        c = 0;
    }
    // h >= p  <=>  h + 5 >= 2^130
    uint64_t g[5];
    c = 5;
    for (int k = 0; k < 5; ++k) {
        g[k] = sum[k] + c;
        c = g[k] >> 26;
        g[k] &= 0x3ffffff;
    }
    if (c) for (int k = 0; k < 5; ++k) sum[k] = g[k];
    // to 128 bits + s
    const uint64_t lo = sum[0] | sum[1] << 26 | sum[2] << 52;
    const uint64_t hi = (sum[2] >> 12) | sum[3] << 14 | sum[4] << 40;
    const uint64_t s_lo = (uint64_t)otk[4] | (uint64_t)otk[5] << 32;
    const uint64_t s_hi = (uint64_t)otk[6] | (uint64_t)otk[7] << 32;
    const uint64_t t_lo = lo + s_lo;
    const uint64_t t_hi = hi + s_hi + (t_lo < lo);
    return t_lo == ((uint64_t)tagw[0] | (uint64_t)tagw[1] << 32) &&
           t_hi == ((uint64_t)tagw[2] | (uint64_t)tagw[3] << 32);
}

// decrypt in place (payload[:0], packet_protector.go:74): lane l takes blocks l, l+64, ...
__device__ __forceinline__ void ctr_decrypt(const uint32_t* te, const uint32_t* rk, const uint32_t nonce[3],
                                            uint8_t* ct, uint64_t ct_len, uint64_t ct_blocks, uint32_t lane) {
    for (uint64_t b = lane; b < ct_blocks; b += 64) {
        const uint32_t cb[4] = {nonce[0], nonce[1], nonce[2], bswap32((uint32_t)(2 + b))};
        uint32_t ks[4], w[4];
        aes_encrypt(te, rk, cb, ks);
        load_block(ct, 16 * b, ct_len, w);
        store_xor(ct, 16 * b, ct_len, w, ks, 4);
    }
}

__device__ __forceinline__ void chacha_decrypt(const uint32_t kw[8], const uint32_t nonce[3], uint8_t* ct,
                                               uint64_t ct_len, uint32_t lane) {
    const uint64_t cblocks = (ct_len + 63) / 64;
    for (uint64_t b = lane; b < cblocks; b += 64) {
        uint32_t ks[16], w[16];
        chacha20_block(kw, (uint32_t)(1 + b), nonce, ks);
#pragma unroll
        for (int q = 0; q < 4; ++q) load_block(ct, 64 * b + 16 * q, ct_len, w + 4 * q);
        store_xor(ct, 64 * b, ct_len, w, ks, 16);
    }
}

// extractCryptoFrames (payload.go:73-112), wave-uniform: the first
// HYOBFS_QUIC_MAX_FRAMES frames to fr, their count (capped or not) to nf
__device__ __forceinline__ int extract_crypto_frames(const uint8_t* ct, uint64_t ct_len, Frame* fr, uint32_t lane,
                                                     uint32_t& nf) {
    int st = HYOBFS_OK;
    Window win{ct, ct_len, ~0ull, 0};
    uint64_t i = 0;
    nf = 0;
    while (i < ct_len && st == HYOBFS_OK) {
        const uint32_t c0 = win.get(i, lane);
        if (c0 <= 1) {   // a run of one-byte PADDING / PING frames
            for (;;) {
                win.fill(i, lane);
                const unsigned long long live = __ballot(i + lane < ct_len && win.mine > 1u);
                if (live) {
                    i += __builtin_ctzll(live);
                    break;
                }
                i += 64;
                if (i >= ct_len) {
                    i = ct_len;
                    break;
                }
            }
            continue;
        }
        uint64_t typ, fo, dl;
        if (!win.varint(i, typ, lane)) { st = HYOBFS_QUIC_ERR_FRAME_EOF; break; }
        if (typ == 0 || typ == 1) continue;
        if (typ != 6) { st = HYOBFS_QUIC_ERR_FRAME_TYPE; break; }
        if (!win.varint(i, fo, lane)) { st = HYOBFS_QUIC_ERR_FRAME_EOF; break; }
        if (!win.varint(i, dl, lane)) { st = HYOBFS_QUIC_ERR_FRAME_EOF; break; }
        if (dl > HYOBFS_QUIC_MAX_CRYPTO_FRAME_LEN) { st = HYOBFS_QUIC_ERR_FRAME_TOO_LARGE; break; }
        if (dl > ct_len - i) { st = HYOBFS_QUIC_ERR_FRAME_EOF; break; }
        if (nf < HYOBFS_QUIC_MAX_FRAMES && lane == 0) fr[nf] = Frame{fo, (uint32_t)dl, (uint32_t)i};
        ++nf;
        i += dl;
    }
    return st;
}

// assembleCryptoFrames (payload.go:116-148) and the copy to the packet's out
// slot; r.out_len = the assembled length even when the slot is too small
__device__ __forceinline__ int assemble_crypto_frames(const Frame* fr, uint16_t* order, uint32_t nf, const uint8_t* ct,
                                                      const OpenArgs& a, uint64_t pk, hyobfs_quic_result& r,
                                                      uint32_t lane, int st) {
    uint64_t out_len = 0, first_off = 0;
    if (st == HYOBFS_OK && nf == 1) {
        out_len = fr[0].len;
        order[0] = 0;
    } else if (st == HYOBFS_OK) {
        // stable rank sort by offset
        for (uint32_t j = lane; j < nf; j += 64) {
            const uint64_t oj = fr[j].off;
            uint32_t rank = 0;
            for (uint32_t k = 0; k < nf; ++k) rank += fr[k].off < oj || (fr[k].off == oj && k < j);
            order[rank] = (uint16_t)j;
        }
        __syncthreads();
        bool gap = false;
        for (uint32_t k = 1 + lane; k < nf; k += 64) {
            const Frame& x = fr[order[k - 1]];
            gap |= fr[order[k]].off != x.off + x.len;
        }
        const Frame& last = fr[order[nf - 1]];
        if (__ballot(gap) || last.off > HYOBFS_QUIC_MAX_CRYPTO_PAYLOAD_LEN ||
            last.off + last.len > HYOBFS_QUIC_MAX_CRYPTO_PAYLOAD_LEN)
            st = HYOBFS_QUIC_ERR_ASSEMBLE;
        else
            out_len = last.off + last.len;
        first_off = fr[order[0]].off;
    }
    if (st == HYOBFS_OK) {
        r.out_len = (uint32_t)out_len;
        if (out_len > a.out_cap[pk]) {
            st = HYOBFS_QUIC_ERR_OUT_CAP;
        } else {
            uint8_t* o = a.out + a.out_off[pk];
            for (uint64_t q = lane; q < (nf > 1 ? first_off : 0); q += 64) o[q] = 0;
            for (uint32_t k = 0; k < nf; ++k) {
                const Frame x = fr[order[k]];
                uint8_t* d = o + (nf > 1 ? x.off : 0);
                const uint8_t* s = ct + x.pos;
                for (uint32_t q = lane; q < x.len; q += 64) d[q] = s[q];
            }
        }
    }
    return st;
}

#ifndef HY_QUIC_MIN_WAVES
#define HY_QUIC_MIN_WAVES 4   // waves per SIMD the open kernel is register-capped for
#endif

template <bool CRYPTO>
__global__ __launch_bounds__(64, HY_QUIC_MIN_WAVES) void quic_open_kernel(OpenArgs a) {
    __shared__ uint32_t te[256];
    __shared__ G128 gtab[7][16];   // GHASH: Shoup tables of H^(2^k)
    __shared__ uint32_t rkl[44];   // AES-128 round keys of the packet's AEAD key
    __shared__ uint32_t hrkl[44];  // ... and of its header-protection key
    __shared__ Frame fr[HYOBFS_QUIC_MAX_FRAMES];
    __shared__ uint16_t order[HYOBFS_QUIC_MAX_FRAMES];
    const uint32_t lane = threadIdx.x & 63;
    aes_table_load(te, lane);

    for (uint64_t pk = blockIdx.x; pk < a.n; pk += gridDim.x) {
        __syncthreads();   // the previous packet's LDS reads are done
        uint8_t* p = a.packets + a.off[pk];
        hyobfs_quic_key key;
        int64_t pn_off, pn_max;
        uint64_t L;
        int st = load_job<CRYPTO>(a, pk, key, pn_off, pn_max, L);
        hyobfs_quic_result r{};
        // UnProtect (packet_protector.go:46-79)
        if (st == HYOBFS_OK && (pn_off < 0 || (uint64_t)pn_off > L || L - (uint64_t)pn_off < 20))
            st = HYOBFS_QUIC_ERR_TOO_SMALL;   // :47-49
        const bool aes = CRYPTO || key.suite == HYOBFS_QUIC_TLS_AES_128_GCM_SHA256;   // Initial packets: AES-128-GCM
        if (st == HYOBFS_OK && !aes && key.suite != HYOBFS_QUIC_TLS_CHACHA20_POLY1305_SHA256)
            st = HYOBFS_QUIC_ERR_SUITE;
        if (st != HYOBFS_OK) {
            if (lane == 0) {
                r.status = st;
                a.res[pk] = r;
            }
            continue;
        }
        uint32_t kw[8], ivw[3], hpw[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) kw[k] = le_word(key.key + 4 * k), hpw[k] = le_word(key.hp + 4 * k);
#pragma unroll
        for (int k = 0; k < 3; ++k) ivw[k] = le_word(key.iv + 4 * k);

        uint32_t mw0, mw1, nonce[3];
        header_mask(aes, te, hrkl, rkl, hpw, kw, p, pn_off, L, lane, mw0, mw1);        // :51-56
        const Unmasked u = unmask_header(p, pn_off, pn_max, mw0, mw1, ivw, nonce);   // :57-72, :93-100
        const uint32_t* rk = rkl;   // round keys live in LDS: registers stay free for occupancy
        r.pn = u.pn;
        r.hdr_len = (uint32_t)u.hdr_len;

        // aead.Open(payload[:0], nonce, payload, hdr) (:74): verify the tag, then decrypt in place
        const uint64_t payload = L - u.hdr_len;
        bool ok = payload >= 16;
        const uint64_t ct_len = ok ? payload - 16 : 0;
        uint8_t* ct = p + u.hdr_len;
        const uint64_t aad_blocks = (u.hdr_len + 15) / 16, ct_blocks = (ct_len + 15) / 16;
        const AeadInput in{p, ct, u, ct_len, aad_blocks, ct_blocks, aad_blocks + ct_blocks + 1};   // + the length block
        const uint64_t nt = lane < in.m ? (in.m - 1 - lane) / 64 + 1 : 0;   // blocks this lane takes
        uint32_t tagw[4];
        if (ok) load_block(p, L - 16, L, tagw);
        if (ok && aes) ok = gcm_tag_ok(te, rk, gtab, nonce, tagw, in, nt, lane);
        else if (ok) ok = poly1305_tag_ok(kw, nonce, tagw, in, nt, lane);
        if (ok) {
            if (aes) ctr_decrypt(te, rk, nonce, ct, ct_len, ct_blocks, lane);
            else chacha_decrypt(kw, nonce, ct, ct_len, lane);
            r.plain_len = (uint32_t)ct_len;
        } else {
            st = HYOBFS_QUIC_ERR_AUTH;   // :75-77
        }
        // the header stays unmasked whatever the AEAD says (packet_protector.go:57-70)
        if (lane == 0) {
            p[0] = (uint8_t)u.first;
            for (uint32_t k = 0; k < u.pn_len; ++k) p[pn_off + k] ^= (uint8_t)(u.pmask >> (8 * k));
        }
        if (CRYPTO && st == HYOBFS_OK) {
            __syncthreads();   // the plaintext stores of every lane are visible below
            uint32_t nf;
            st = extract_crypto_frames(ct, ct_len, fr, lane, nf);   // payload.go:51-54, 73-112
            if (st == HYOBFS_OK && nf == 0) st = HYOBFS_QUIC_ERR_ASSEMBLE;   // payload.go:55-58
            if (st == HYOBFS_OK && nf > HYOBFS_QUIC_MAX_FRAMES) st = HYOBFS_QUIC_ERR_FRAMES;
            __syncthreads();
            st = assemble_crypto_frames(fr, order, nf, ct, a, pk, r, lane, st);   // payload.go:116-148
            __syncthreads();   // fr / order are reused by the next packet
        }
        if (lane == 0) {
            r.status = st;
            a.res[pk] = r;
        }
    }
}

// one workgroup per packet, grid-stride past 2^20
inline uint32_t grid_for(uint64_t n) { return (uint32_t)(n < (1u << 20) ? n : (1u << 20)); }

}  // namespace quic
}  // namespace hyobfs

// ------------------------------------------------------------------ C ABI
using namespace hyobfs::quic;

namespace {

// host HKDF over byte strings (secret <= 64 bytes)
int expand_label(const uint8_t* secret, size_t sl, const char* label, const uint8_t* ctx, size_t cl, uint8_t* out,
                 size_t L) {
    const size_t ll = std::strlen(label);
    if (sl > 64 || 6 + ll > 255 || cl > 255 || L > 255 * 32 || (L && !out)) return HYOBFS_ERR_INVALID;
    std::vector<uint8_t> info{(uint8_t)(L >> 8), (uint8_t)L, (uint8_t)(6 + ll), 't', 'l', 's', '1', '3', ' '};
    info.insert(info.end(), label, label + ll);
    info.push_back((uint8_t)cl);
    if (cl) info.insert(info.end(), ctx, ctx + cl);
    uint8_t t[32];
    size_t done = 0;
    std::vector<uint8_t> msg;
    for (uint32_t i = 1; done < L; ++i) {
        if (i == 1) msg.clear();   // T(0) is empty, T(i) = HMAC(T(i-1) || info || i)
        else msg.assign(t, t + 32);
        msg.insert(msg.end(), info.begin(), info.end());
        msg.push_back((uint8_t)i);
        hmac_host(secret, sl, msg.data(), msg.size(), t);
        const size_t k = L - done < 32 ? L - done : 32;
        std::memcpy(out + done, t, k);
        done += k;
    }
    return HYOBFS_OK;
}

}  // namespace

extern "C" {

int hyobfs_quic_parse_initial_header(const uint8_t* data, size_t len, hyobfs_quic_header* out) {
    if (!out || (len && !data)) return HYOBFS_ERR_INVALID;
    const int st = parse_initial_header(data, len, *out);
    if (st != HYOBFS_OK) std::memset(out, 0, sizeof(*out));   // a failed parse leaves nothing behind
    return st;
}

int hyobfs_quic_hkdf_expand_label(const uint8_t* secret, size_t secret_len, const char* label,
                                  const uint8_t* context, size_t context_len, uint8_t* out, size_t length) {
    if (!secret || !label || (context_len && !context)) return HYOBFS_ERR_INVALID;
    return expand_label(secret, secret_len, label, context, context_len, out, length);
}

int hyobfs_quic_initial_secret(const uint8_t* dcid, size_t dcid_len, uint32_t version, int server,
                               uint8_t out[32]) {
    if (!out || (dcid_len && !dcid)) return HYOBFS_ERR_INVALID;
    uint8_t prk[32];
    hmac_host(get_salt(version), 20, dcid, dcid_len, prk);   // HKDF-Extract(salt, dcid)
    return expand_label(prk, 32, server ? "server in" : "client in", nullptr, 0, out, 32);
}

int hyobfs_quic_new_protection_key(uint16_t suite, const uint8_t* secret, size_t secret_len, uint32_t version,
                                   hyobfs_quic_key* out) {
    if (!secret || !out) return HYOBFS_ERR_INVALID;
    size_t kl;
    if (suite == HYOBFS_QUIC_TLS_AES_128_GCM_SHA256) kl = 16;
    else if (suite == HYOBFS_QUIC_TLS_CHACHA20_POLY1305_SHA256) kl = 32;
    else return HYOBFS_QUIC_ERR_SUITE;
    const bool v2 = version == HYOBFS_QUIC_V2;   // quic.go:38-59
    std::memset(out, 0, sizeof(*out));
    out->suite = suite;
    int rc = expand_label(secret, secret_len, v2 ? "quicv2 key" : "quic key", nullptr, 0, out->key, kl);
    if (rc == HYOBFS_OK) rc = expand_label(secret, secret_len, v2 ? "quicv2 iv" : "quic iv", nullptr, 0, out->iv, 12);
    if (rc == HYOBFS_OK) rc = expand_label(secret, secret_len, v2 ? "quicv2 hp" : "quic hp", nullptr, 0, out->hp, kl);
    return rc;
}

int hyobfs_quic_unprotect_batch(uint8_t* packets, const uint64_t* off, const uint32_t* len, uint64_t n,
                                const hyobfs_quic_key* keys, uint32_t key_stride, const int64_t* pn_offset,
                                const int64_t* pn_max, hyobfs_quic_result* res, void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!packets || !off || !len || !keys || !pn_offset || !res || key_stride > 1) return HYOBFS_ERR_INVALID;
    OpenArgs a{packets, off, len, n, keys, key_stride, pn_offset, pn_max, nullptr, res, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(quic_open_kernel<false>, dim3(grid_for(n)), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    return hyobfs::hy_status(hipGetLastError());
}

uint64_t hyobfs_quic_workspace_size(uint64_t n) { return n * sizeof(Job); }

int hyobfs_quic_read_crypto_payload_batch(uint8_t* packets, const uint64_t* off, const uint32_t* len, uint64_t n,
                                          uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                                          hyobfs_quic_result* res, void* workspace, void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!packets || !off || !len || !out || !out_off || !out_cap || !res || !workspace) return HYOBFS_ERR_INVALID;
    static const PrepConsts consts = make_prep_consts();
    Job* jobs = static_cast<Job*>(workspace);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(quic_prep_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, packets, off, len, n,
                       jobs, consts);
    if (hipGetLastError() != hipSuccess) return HYOBFS_ERR_HIP;
    OpenArgs a{packets, off, len, n, nullptr, 0, nullptr, nullptr, jobs, res, out, out_off, out_cap};
    hipLaunchKernelGGL(quic_open_kernel<true>, dim3(grid_for(n)), dim3(64), 0, s, a);
    return hyobfs::hy_status(hipGetLastError());
}

}  // extern "C"
