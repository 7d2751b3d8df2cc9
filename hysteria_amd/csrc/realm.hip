// realm.hip -- realm hole-punch packet mask (include/hyobfs_realm.h).
//
// mask = SHA-256(obfsKey(32) || salt(8)) (punch.go:133-141): a 40-byte message,
// so one SHA-256 compression of a single padded block (FIPS 180-4).  The match
// kernel gives one thread to each received datagram and walks the registered
// attempts in order (punch_conn.go:146-165); only the first 25 plain bytes
// (magic, type, nonce) decide, so it loads 33 bytes per datagram.  The host
// entry points (encode / decode / mask) share the same code (sha256.h).
#include "kernels.h"
#include "../../include/hyobfs_realm.h"
#include "sha256.h"

namespace hyobfs {

// SHA-256 of the 40-byte message key || salt: one compression of the padded block.
HY_HD void sha256_key_salt(const uint8_t key[32], const uint8_t salt[8], uint8_t mask[32]) {
    uint32_t w[16], st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = be32(key + 4 * i);
#pragma unroll
    for (int i = 0; i < 2; ++i) w[8 + i] = be32(salt + 4 * i);
    w[10] = 0x80000000u;   // the 0x80 terminator
#pragma unroll
    for (int i = 11; i < 15; ++i) w[i] = 0;
    w[15] = 40 * 8;        // message length in bits
    sha256_init(st);
    sha256_compress(st, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) put_be32(mask + 4 * i, st[i]);
}

constexpr uint8_t kPunchMagic[8] = {'H', 'Y', 'R', 'L', 'M', 'v', '1', 0};

// DecodePunchPacket's checks after the length checks (punch.go:86-99), on the first 25 plain bytes.
HY_HD int punch_check(const uint8_t head[HYOBFS_PUNCH_HEADER_LEN], const uint8_t* nonce) {
    for (int i = 0; i < 8; ++i)
        if (head[i] != kPunchMagic[i]) return HYOBFS_PUNCH_ERR_BAD_MAGIC;
    if (head[8] != HYOBFS_PUNCH_HELLO && head[8] != HYOBFS_PUNCH_ACK) return HYOBFS_PUNCH_ERR_UNKNOWN_TYPE;
    for (int i = 0; i < HYOBFS_PUNCH_NONCE_LEN; ++i)
        if (head[9 + i] != nonce[i]) return HYOBFS_PUNCH_ERR_NONCE_MISMATCH;
    return HYOBFS_OK;
}

__global__ __launch_bounds__(256) void punch_match_kernel(const uint8_t* in, const uint64_t* in_off,
                                                          const uint32_t* in_len, uint64_t n,
                                                          const hyobfs_punch_attempt* attempts, uint32_t m,
                                                          int32_t* match, uint8_t* type, uint32_t* padding) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t len = in_len[i];
    int32_t hit = -1;
    uint8_t ty = 0;
    if (len >= HYOBFS_PUNCH_MIN_WIRE_LEN && len <= HYOBFS_PUNCH_MAX_WIRE_LEN) {
        const uint8_t* p = in + in_off[i];
        uint8_t salt[8], enc[HYOBFS_PUNCH_HEADER_LEN];
        for (int k = 0; k < 8; ++k) salt[k] = p[k];
        for (int k = 0; k < HYOBFS_PUNCH_HEADER_LEN; ++k) enc[k] = p[8 + k];
        for (uint32_t j = 0; j < m && hit < 0; ++j) {
            const hyobfs_punch_attempt& a = attempts[j];
            uint8_t mask[32], head[HYOBFS_PUNCH_HEADER_LEN];
            sha256_key_salt(a.key, salt, mask);
            for (int k = 0; k < HYOBFS_PUNCH_HEADER_LEN; ++k) head[k] = enc[k] ^ mask[k];
            if (punch_check(head, a.nonce) == HYOBFS_OK) {
                hit = (int32_t)j;
                ty = head[8];
            }
        }
    }
    match[i] = hit;
    if (type) type[i] = ty;
    if (padding) padding[i] = hit >= 0 ? len - HYOBFS_PUNCH_MIN_WIRE_LEN : 0u;
}

hipError_t launch_punch_match(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint64_t n,
                              const hyobfs_punch_attempt* attempts, uint32_t m, int32_t* match, uint8_t* type,
                              uint32_t* padding, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(punch_match_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, in, in_off, in_len, n,
                       attempts, m, match, type, padding);
    return hipGetLastError();
}

}  // namespace hyobfs

extern "C" {

int hyobfs_punch_match_batch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint64_t n,
                             const hyobfs_punch_attempt* attempts, uint32_t m, int32_t* match, uint8_t* type,
                             uint32_t* padding, void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!in || !in_off || !in_len || !match || (m && !attempts)) return HYOBFS_ERR_INVALID;
    return hyobfs::hy_status(hyobfs::launch_punch_match(in, in_off, in_len, n, attempts, m, match, type, padding,
                                                        static_cast<hipStream_t>(stream)));
}

void hyobfs_punch_mask(const uint8_t key[32], const uint8_t salt[8], uint8_t mask[32]) {
    hyobfs::sha256_key_salt(key, salt, mask);
}

int64_t hyobfs_punch_encode(uint8_t type, const hyobfs_punch_attempt* a, const uint8_t salt[8],
                            const uint8_t* padding, size_t padding_len, uint8_t* out, size_t cap) {
    if (type != HYOBFS_PUNCH_HELLO && type != HYOBFS_PUNCH_ACK) return HYOBFS_PUNCH_ERR_UNKNOWN_TYPE;
    if (!a || !salt || !out || padding_len > HYOBFS_PUNCH_MAX_PADDING || (padding_len && !padding))
        return HYOBFS_ERR_INVALID;
    const size_t total = HYOBFS_PUNCH_MIN_WIRE_LEN + padding_len;
    if (cap < total) return HYOBFS_ERR_INVALID;
    uint8_t mask[32];
    hyobfs::sha256_key_salt(a->key, salt, mask);
    std::memcpy(out, salt, HYOBFS_PUNCH_SALT_LEN);
    uint8_t* plain = out + HYOBFS_PUNCH_SALT_LEN;
    std::memcpy(plain, hyobfs::kPunchMagic, 8);
    plain[8] = type;
    std::memcpy(plain + 9, a->nonce, HYOBFS_PUNCH_NONCE_LEN);
    if (padding_len) std::memcpy(plain + HYOBFS_PUNCH_HEADER_LEN, padding, padding_len);
    for (size_t i = 0; i < HYOBFS_PUNCH_HEADER_LEN + padding_len; ++i) plain[i] ^= mask[i % 32];
    return (int64_t)total;
}

int hyobfs_punch_decode(const uint8_t* packet, size_t len, const hyobfs_punch_attempt* a, uint8_t* type,
                        uint32_t* padding_len) {
    if (len < HYOBFS_PUNCH_MIN_WIRE_LEN) return HYOBFS_PUNCH_ERR_TOO_SHORT;
    if (len > HYOBFS_PUNCH_MAX_WIRE_LEN) return HYOBFS_PUNCH_ERR_TOO_LONG;
    if (!packet || !a) return HYOBFS_ERR_INVALID;
    uint8_t mask[32], head[HYOBFS_PUNCH_HEADER_LEN];
    hyobfs::sha256_key_salt(a->key, packet, mask);
    for (int k = 0; k < HYOBFS_PUNCH_HEADER_LEN; ++k) head[k] = packet[8 + k] ^ mask[k];
    const int rc = hyobfs::punch_check(head, a->nonce);
    if (rc != HYOBFS_OK) return rc;
    if (type) *type = head[8];
    if (padding_len) *padding_len = (uint32_t)(len - HYOBFS_PUNCH_MIN_WIRE_LEN);
    return HYOBFS_OK;
}

}  // extern "C"
