// udpmsg.hip -- the UDP relay message over batches (include/hyobfs_udpmsg.h, which
// states the rules): parse, fragment-and-serialise, reassemble.
//
// Reference: apernet/hysteria core/internal/protocol/proxy.go:151-256
// (UDPMessage, ParseUDPMessage, varintPut), core/internal/frag/frag.go
// (FragUDPMessage, Defragger), core/server/udp.go:207-235 (sendMessageAutoFrag).
//
//   udp_parse_kernel     one thread per datagram (the shape of gecko_parse_kernel).
//
//   hyobfs_udp_frag_batch is four launches:
//   udp_plan_kernel      one thread per message: rule A's datagram count and byte
//                        count, summed per tile of 256 messages.
//   udp_scan_kernel      one workgroup: exclusive scan of the two tile-sum arrays
//                        in place, 256 tiles per pass (the sums of the passes before are
//                        carried along), the totals at [ntiles].
//   udp_index_kernel     one thread per message: its place in both running sums
//                        (tile prefix + a workgroup scan), the capacity rule, and
//                        status / first / dgram_off / dgram_len / totals.
//   udp_write_kernel     THE HOT PATH.  One wave per group of 64 consecutive
//                        messages, whose output is one contiguous byte range.  The
//                        wave keeps the 64 plans in LDS and sweeps the range in
//                        aligned 16-byte windows, 64 windows per step, each lane
//                        building one window in registers: the bytes a window takes
//                        from a payload come from ONE 16-byte load at the matching
//                        (unaligned) source address, shifted into place when the
//                        window also holds other bytes; header bytes (the eight
//                        fixed ones and the varint, built in registers, and the
//                        address, loaded the same way) are merged into the same
//                        window.  So every payload byte is read once and every
//                        output byte written once, in whole aligned 16-byte stores;
//                        only a group's first and last window, which it may share
//                        with the neighbouring groups, are written under a byte
//                        mask.  Loads are clamped to the region they read from
//                        (payload, address), so nothing outside the stated inputs
//                        is touched.
//
//   udp_assemble_kernel  four messages per wave, 16 lanes each, for lists of at most 16
//                        fragments (nearly all: a message is one or two datagrams): each
//                        lane checks one fragment, a 16-lane scan gives the slice offsets
//                        (kept in LDS), and the 16 lanes sweep the message's output range
//                        in aligned 16-byte windows with the same store discipline
//                        (masked first / last window).  A longer list (up to 255) is then
//                        taken by the whole wave, four fragments per lane.
#include "salamander_device.h"

#define HY_UDP_FN __host__ __device__ __forceinline__
#include "udpmsg_rules.h"

namespace hyobfs {
namespace udpmsg {

// messages per tile-sum entry (one workgroup of the plan / index kernels) and tiles per pass of the scan: whole
// waves.  The CPU test tier also builds them small, so that a batch beyond one pass stays cheap there.
#ifndef HY_UDP_TILE_MSGS
#define HY_UDP_TILE_MSGS 256
#endif
#ifndef HY_UDP_SCAN_TILES
#define HY_UDP_SCAN_TILES 256
#endif
constexpr int kTileMsgs = HY_UDP_TILE_MSGS, kScanTiles = HY_UDP_SCAN_TILES;
static_assert(kTileMsgs % 64 == 0 && kTileMsgs <= 1024 && kScanTiles % 64 == 0 && kScanTiles <= 1024, "whole waves");
constexpr int kGroupMsgs = 64;   // messages per wave of the write kernel
constexpr int kWaves = 4;        // waves per workgroup (write, assemble)
constexpr int kU = 4;            // windows per lane and step: all loads of a step are issued before its stores

struct FragArgs {
    const uint8_t* data;
    const uint64_t* data_off;
    const uint32_t* data_len;
    const hyobfs_udp_meta* meta;
    const uint8_t* addrs;
    uint64_t n;
    uint8_t* out;
    uint64_t out_cap;
    uint64_t* dgram_off;
    uint32_t* dgram_len;
    uint64_t dgram_cap;
    uint64_t* first;
    int32_t* status;
    uint64_t* totals;
    uint64_t* tile_bytes;    // workspace: ntiles + 1
    uint64_t* tile_dgrams;   // workspace: ntiles + 1
    uint64_t* group_off;     // workspace: byte offset in `out` of each group of 64 messages
};

__device__ __forceinline__ SendPlan plan_of(const FragArgs& A, uint64_t i) {
    return send_plan(A.meta[i].addr_len, A.data_len[i], A.meta[i].max_size);
}

__global__ __launch_bounds__(256) void udp_parse_kernel(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                                        uint64_t n, hyobfs_udp_parsed* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    hyobfs_udp_parsed r;
    parse(in + in_off[i], in_len[i], &r);
    out[i] = r;
}

__global__ __launch_bounds__(kTileMsgs) void udp_plan_kernel(FragArgs A) {
    __shared__ uint64_t s_b[kTileMsgs / 64], s_d[kTileMsgs / 64];
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * kTileMsgs + threadIdx.x;
    uint64_t b = 0, d = 0;
    if (i < A.n) {
        const SendPlan p = plan_of(A, i);
        b = p.bytes;
        d = p.count;
    }
    b = wave_sum(b);
    d = wave_sum(d);
    if (lane == 0) {
        s_b[wid] = b;
        s_d[wid] = d;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        b = d = 0;
        for (int w = 0; w < kTileMsgs / 64; ++w) {
            b += s_b[w];
            d += s_d[w];
        }
        A.tile_bytes[blockIdx.x] = b;
        A.tile_dgrams[blockIdx.x] = d;
    }
}

// Exclusive scan of a[0, ntiles) and b[0, ntiles) in place, the totals at [ntiles]; one workgroup.
__global__ __launch_bounds__(kScanTiles) void udp_scan_kernel(uint64_t* a, uint64_t* b, uint64_t ntiles) {
    __shared__ uint64_t s_a[kScanTiles / 64], s_b[kScanTiles / 64];
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint64_t ca = 0, cb = 0;   // the sums of the passes before this one
    for (uint64_t base = 0; base < ntiles; base += kScanTiles) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t xa = i < ntiles ? a[i] : 0, xb = i < ntiles ? b[i] : 0;
        const uint64_t ia = wave_incl_scan(xa, (int)lane), ib = wave_incl_scan(xb, (int)lane);
        if (lane == 63) {
            s_a[wid] = ia;
            s_b[wid] = ib;
        }
        __syncthreads();
        uint64_t pa = 0, pb = 0, ta = 0, tb = 0;
        for (uint32_t w = 0; w < kScanTiles / 64; ++w) {
            pa += w < wid ? s_a[w] : 0;
            pb += w < wid ? s_b[w] : 0;
            ta += s_a[w];
            tb += s_b[w];
        }
        if (i < ntiles) {
            a[i] = ca + pa + ia - xa;
            b[i] = cb + pb + ib - xb;
        }
        ca += ta;
        cb += tb;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a[ntiles] = ca;
        b[ntiles] = cb;
    }
}

__global__ __launch_bounds__(kTileMsgs) void udp_index_kernel(FragArgs A) {
    __shared__ uint64_t s_b[kTileMsgs / 64], s_d[kTileMsgs / 64];
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * kTileMsgs + threadIdx.x;
    SendPlan p{};
    if (i < A.n) p = plan_of(A, i);
    const uint64_t ib = wave_incl_scan((uint64_t)p.bytes, (int)lane), id = wave_incl_scan((uint64_t)p.count, (int)lane);
    if (lane == 63) {
        s_b[wid] = ib;
        s_d[wid] = id;
    }
    __syncthreads();
    uint64_t B = A.tile_bytes[blockIdx.x], D = A.tile_dgrams[blockIdx.x];   // bytes / datagrams of the messages before i
    for (uint32_t w = 0; w < wid; ++w) {
        B += s_b[w];
        D += s_d[w];
    }
    B += ib - p.bytes;
    D += id - p.count;
    if (i >= A.n) return;
    // the capacity rule: the sums through i must fit
    const int32_t st = (B + p.bytes > A.out_cap || D + p.count > A.dgram_cap) ? HYOBFS_UDP_ERR_CAP : p.status;
    A.status[i] = st;
    A.first[i] = D;
    if ((i & (kGroupMsgs - 1)) == 0) A.group_off[i / kGroupMsgs] = B;
    if (i == A.n - 1) {
        A.first[A.n] = D + p.count;
        A.totals[0] = B + p.bytes;
        A.totals[1] = D + p.count;
    }
    if (st != HYOBFS_OK) return;
    for (uint32_t k = 0; k < p.count; ++k) {
        const uint32_t at = k * p.stride;
        A.dgram_off[D + k] = B + at;
        A.dgram_len[D + k] = min(p.stride, p.bytes - at);
    }
}

// ---------------------------------------------------------------- windows
// (shift_into_place, region_bytes and store_window: salamander_device.h)

// p / d for p < 2^21 (a message's output: at most 255 headers of at most 4096 bytes, and its data) and
// d >= 9: the float quotient is off by at most one, which the two compares put right
__device__ __forceinline__ uint32_t div_small(uint32_t p, uint32_t d) {
    uint32_t q = (uint32_t)((float)p * (1.0f / (float)d));
    q -= q * d > p;
    q += (q + 1) * d <= p;
    return q;
}

// the eight fixed bytes and the varint of a datagram's header (proxy.go:183-187)
__device__ __forceinline__ u128 fixed_header(uint32_t session, uint32_t pid, uint32_t k, uint32_t count,
                                             uint32_t addr_len) {
    const uint64_t lo = (uint64_t)__builtin_bswap32(session) | (uint64_t)(((pid >> 8) & 0xffu) | ((pid & 0xffu) << 8)) << 32 |
                        (uint64_t)k << 48 | (uint64_t)count << 56;
    const uint32_t vl = varint_len(addr_len);
    uint64_t hi = 0;
    for (uint32_t j = 0; j < vl; ++j) hi |= (uint64_t)varint_byte(addr_len, vl, j) << (8 * j);
    return (u128)hi << 64 | lo;
}

// ---------------------------------------------------------------- the write kernel
// The plans of a wave's 64 messages.  Positions are "virtual": byte offsets from
// the 16-aligned address at or below the group's first output byte, so a window
// index is a virtual position / 16 and off[0] is the misalignment (0..15).
struct FragGroup {
    uint32_t off[kGroupMsgs + 1];   // where each message's output starts; [64]: where the group's ends
    uint32_t stride[kGroupMsgs], hdr[kGroupMsgs], max_payload[kGroupMsgs], count[kGroupMsgs];
    uint32_t session[kGroupMsgs], pid[kGroupMsgs], addr_len[kGroupMsgs];
    uint64_t addr_off[kGroupMsgs], data_off[kGroupMsgs];
};

// the window at virtual position a: its bytes in r, which of them belong to the group in cov
__device__ __forceinline__ void frag_window(const FragArgs& A, const FragGroup& G, uint32_t a, u128& r, uint32_t& cov) {
    const uint32_t stop = min(a + 16u, G.off[kGroupMsgs]);
    uint32_t pos = max(a, G.off[0]);
    uint32_t m = 0;   // the last message that starts at or before pos
#pragma unroll
    for (uint32_t step = kGroupMsgs / 2; step; step >>= 1) m = G.off[m + step] <= pos ? m + step : m;
    r = 0;
    cov = 0;
    while (pos < stop) {
        while (G.off[m + 1] <= pos) ++m;   // also steps over messages that produce nothing
        const uint32_t mo = G.off[m], stride = G.stride[m], hdr = G.hdr[m];
        const uint32_t k = div_small(pos - mo, stride);  // the fragment and
        const uint32_t fs = mo + k * stride;             // where it starts
        const uint32_t q = pos - fs;
        const uint32_t addr_len = G.addr_len[m], fixed = hdr - addr_len;   // 8 + the varint's bytes
        uint32_t re;
        u128 X;
        if (q >= hdr) {   // payload
            const uint32_t rs = fs + hdr;
            re = min(fs + stride, G.off[m + 1]);
            const uint8_t* src = A.data + G.data_off[m] + (uint64_t)k * G.max_payload[m];
            if (pos == a && re >= a + 16u) {   // the whole window: nearly every window of a batch
                r = load16u(src + (a - rs));
                cov = 0xFFFFu;
                return;
            }
            X = region_bytes(src, re - rs, (int)a - (int)rs, pos - a, min(re, stop) - a);
        } else if (q >= fixed) {   // address
            const uint32_t rs = fs + fixed;
            re = fs + hdr;
            X = region_bytes(A.addrs + G.addr_off[m], addr_len, (int)a - (int)rs, pos - a, min(re, stop) - a);
        } else {
            re = fs + fixed;
            X = shift_into_place(fixed_header(G.session[m], G.pid[m], k, G.count[m], addr_len), (int)a - (int)fs, 0);
        }
        const uint32_t se = min(re, stop);
        r |= X & bytemask(pos - a, se - a);
        cov |= ((1u << (se - pos)) - 1u) << (pos - a);
        pos = se;
    }
}

__global__ __launch_bounds__(kGroupMsgs* kWaves) void udp_write_kernel(FragArgs A) {
    __shared__ FragGroup s_g[kWaves];
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t g = (uint64_t)blockIdx.x * kWaves + wid;
    if (g * kGroupMsgs >= A.n) return;   // whole waves
    FragGroup& G = s_g[wid];
    const uint64_t i = g * kGroupMsgs + lane;
    uint32_t bytes = 0;
    if (i < A.n && A.status[i] == HYOBFS_OK) {
        const hyobfs_udp_meta m = A.meta[i];
        const SendPlan p = send_plan(m.addr_len, A.data_len[i], m.max_size);
        bytes = p.bytes;
        G.stride[lane] = p.stride;
        G.hdr[lane] = p.hdr;
        G.max_payload[lane] = p.max_payload;
        G.count[lane] = p.count;
        G.session[lane] = m.session_id;
        G.pid[lane] = p.count == 1 ? 0u : m.packet_id;   // A2 / A3
        G.addr_len[lane] = m.addr_len;
        G.addr_off[lane] = m.addr_off;
        G.data_off[lane] = A.data_off[i];
    }
    // the messages written are a prefix of those that produce something (the capacity rule), so
    // the group's output is one range that starts at group_off[g]
    const uint64_t gbase = uni64(A.group_off[g]);
    const uint32_t vb = (uint32_t)((reinterpret_cast<uintptr_t>(A.out) + gbase) & 15u);
    const uint32_t inc = wave_incl_scan32(bytes, (int)lane);
    G.off[lane] = vb + inc - bytes;
    if (lane == 63) G.off[kGroupMsgs] = vb + inc;
    hy_wave_sync();
    const uint32_t end = uni32(G.off[kGroupMsgs]);
    if (end == vb) return;   // nothing of this group is written
    uint8_t* const wbase = A.out + gbase - vb;   // 16-aligned
    const uint32_t nwin = (end + 15u) >> 4;
    for (uint32_t T = 0; T < nwin; T += 64 * kU) {
        u128 r[kU];
        uint32_t cov[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const uint32_t t = T + 64 * u + lane;
            r[u] = 0;
            cov[u] = 0;
            if (t < nwin) frag_window(A, G, 16 * t, r[u], cov[u]);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) store_window(wbase + 16ull * (T + 64 * u + lane), r[u], cov[u]);
    }
}

// ---------------------------------------------------------------- assemble
struct AsmArgs {
    const uint8_t* in;
    const uint64_t* in_off;
    const hyobfs_udp_parsed* parsed;
    uint64_t n;
    const uint32_t* frag_idx;
    const uint64_t* msg_first;
    uint64_t m;
    uint8_t* out;
    const uint64_t* out_off;
    const uint32_t* out_cap;
    uint32_t* out_len;
    int32_t* status;
};

constexpr uint32_t kNoSlice = 0xFFFFFFFFu;
constexpr int kAsmLanes = 16;                   // lanes that share a message with a short list
constexpr int kAsmPerWave = 64 / kAsmLanes;     // messages per wave
// pre[c]: where slice c starts in the message; pre[count] = the total; beyond: kNoSlice.  src[c]: where it
// starts in `in`.  A list of at most kAsmLanes slices lives in the small form, a longer one in the large.
struct AsmSmall {
    uint32_t pre[kAsmPerWave][kAsmLanes + 1];
    uint64_t src[kAsmPerWave][kAsmLanes];
};
struct AsmLarge {
    uint32_t pre[257];
    uint64_t src[256];
};

// The sweep of one message's output [out + o, + total) in aligned 16-byte windows by LANES lanes (this one
// is lane `sl` of them), kU windows per lane and step.  The slices are pre / src as above, 2 * TOP >= their
// number.  No wavefront operation: the lanes of a wave may be at work on different messages.
template <uint32_t LANES, uint32_t TOP>
__device__ __forceinline__ void asm_sweep(const uint8_t* __restrict__ in, uint8_t* out, uint64_t o, uint64_t total,
                                          const uint32_t* pre, const uint64_t* src, uint32_t sl) {
    const uint32_t vb = (uint32_t)((reinterpret_cast<uintptr_t>(out) + o) & 15u);
    uint8_t* const wbase = out + o - vb;   // 16-aligned
    const uint64_t end = (uint64_t)vb + total;
    const uint32_t nwin = (uint32_t)((end + 15u) >> 4);
    for (uint32_t T = 0; T < nwin; T += LANES * kU) {
        u128 r[kU];
        uint32_t cov[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const uint32_t t = T + LANES * u + sl;
            r[u] = 0;
            cov[u] = 0;
            if (t >= nwin) continue;
            const uint64_t a = 16ull * t, stop = min(a + 16u, end);
            uint64_t pos = max(a, (uint64_t)vb);
            uint32_t q = 0;   // the last slice that starts at or before pos
#pragma unroll
            for (uint32_t step = TOP; step; step >>= 1) q = pre[q + step] <= (uint32_t)(pos - vb) ? q + step : q;
            while (pos < stop) {
                const uint32_t p = (uint32_t)(pos - vb);
                while (pre[q + 1] <= p) ++q;
                const uint32_t rs = pre[q], re = pre[q + 1];
                const uint64_t se = min((uint64_t)vb + re, stop);
                const int base = (int)((int64_t)a - (int64_t)vb - (int64_t)rs);   // -15 .. re - rs - 1
                const uint8_t* s = in + src[q];
                if (pos == a && se == a + 16u) {
                    r[u] = load16u(s + base);
                    cov[u] = 0xFFFFu;
                    break;
                }
                const u128 X = region_bytes(s, re - rs, base, (uint32_t)(pos - a), (uint32_t)(se - a));
                r[u] |= X & bytemask((uint32_t)(pos - a), (uint32_t)(se - a));
                cov[u] |= ((1u << (uint32_t)(se - pos)) - 1u) << (uint32_t)(pos - a);
                pos = se;
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) store_window(wbase + 16ull * (T + LANES * u + sl), r[u], cov[u]);
    }
}

// One message with a list of 17 to 255 slices, by a whole wave: lane l holds slices 4l .. 4l + 3.
__device__ __forceinline__ void assemble_large(const AsmArgs& A, AsmLarge& G, uint64_t j, uint64_t b, uint32_t cnt,
                                               uint32_t lane) {
    uint32_t len[4] = {0, 0, 0, 0}, bad = 0;
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t c = 4 * lane + k;
        if (c < cnt) {
            const uint32_t idx = A.frag_idx[b + c];
            if (idx >= A.n || A.parsed[idx].status != HYOBFS_OK) {
                bad = 1;
            } else {
                len[k] = A.parsed[idx].data_len;
                G.src[c] = A.in_off[idx] + A.parsed[idx].data_off;
                sum += len[k];
            }
        }
    }
    const uint64_t inc = wave_incl_scan(sum, (int)lane);
    const uint64_t total = wave_sum(sum);
    const bool any_bad = wave_sum((uint64_t)bad) != 0;
    const int32_t st = any_bad ? HYOBFS_UDP_ERR_PLAN : total > A.out_cap[j] ? HYOBFS_UDP_ERR_CAP : HYOBFS_OK;
    if (lane == 0) {
        A.status[j] = st;
        A.out_len[j] = st == HYOBFS_OK ? (uint32_t)total : 0u;
    }
    if (st == HYOBFS_OK && total != 0) {   // wave-uniform
        uint32_t run = (uint32_t)(inc - sum);   // total <= out_cap[j] < 2^32
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t c = 4 * lane + k;
            G.pre[c] = c <= cnt ? run : kNoSlice;
            run += len[k];
        }
        if (lane == 63) G.pre[256] = kNoSlice;
        hy_wave_sync();
        asm_sweep<64, 128>(A.in, A.out, A.out_off[j], total, G.pre, G.src, lane);
    }
    hy_wave_sync();   // G is reused for the wave's next long list
}

__global__ __launch_bounds__(64 * kWaves) void udp_assemble_kernel(AsmArgs A) {
    __shared__ AsmSmall s_small[kWaves];
    __shared__ AsmLarge s_large[kWaves];
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t sub = lane / kAsmLanes, sl = lane % kAsmLanes;
    const uint64_t j0 = ((uint64_t)blockIdx.x * kWaves + wid) * kAsmPerWave;
    if (j0 >= A.m) return;   // whole waves
    // ---- four messages per wave, 16 lanes each: lane sl of a message holds its slice sl
    const uint64_t j = j0 + sub;
    const bool live = j < A.m;
    uint64_t b = 0, e = 0;
    if (live) {
        b = A.msg_first[j];
        e = A.msg_first[j + 1];
    }
    const bool list_ok = e > b && e - b <= HYOBFS_UDP_MAX_FRAGS;
    const uint32_t cnt = list_ok ? (uint32_t)(e - b) : 0u;
    const bool small = live && cnt <= kAsmLanes;   // a list that cannot be assembled at all is answered here too
    uint32_t len = 0, bad = 0;
    uint64_t src = 0;
    if (small && sl < cnt) {
        const uint32_t idx = A.frag_idx[b + sl];
        if (idx >= A.n || A.parsed[idx].status != HYOBFS_OK) {
            bad = 1;
        } else {
            len = A.parsed[idx].data_len;
            src = A.in_off[idx] + A.parsed[idx].data_off;
        }
    }
    uint64_t inc = len;   // inclusive scan and "any" over the message's 16 lanes
#pragma unroll
    for (uint32_t d = 1; d < kAsmLanes; d <<= 1) {
        const uint64_t y = __shfl_up(inc, d, 64);
        const uint32_t z = __shfl_xor(bad, (int)d, 64);
        if (sl >= d) inc += y;
        bad |= z;
    }
    const uint64_t total = __shfl(inc, (int)(lane | (kAsmLanes - 1)), 64);
    int32_t st = HYOBFS_OK;
    if (small) {
        st = (!list_ok || bad) ? HYOBFS_UDP_ERR_PLAN : total > A.out_cap[j] ? HYOBFS_UDP_ERR_CAP : HYOBFS_OK;
        if (sl == 0) {
            A.status[j] = st;
            A.out_len[j] = st == HYOBFS_OK ? (uint32_t)total : 0u;
        }
    }
    AsmSmall& S = s_small[wid];
    S.pre[sub][sl] = sl <= cnt ? (uint32_t)(inc - len) : kNoSlice;   // [cnt] = the total (len is 0 there)
    if (sl == kAsmLanes - 1) S.pre[sub][kAsmLanes] = cnt == kAsmLanes ? (uint32_t)inc : kNoSlice;
    S.src[sub][sl] = src;
    hy_wave_sync();
    if (small && st == HYOBFS_OK && total != 0)
        asm_sweep<kAsmLanes, kAsmLanes / 2>(A.in, A.out, A.out_off[j], total, S.pre[sub], S.src[sub], sl);
    // ---- the wave's messages with longer lists, one after the other by the whole wave
    const uint32_t long_cnt = live && !small ? cnt : 0u;
    for (uint32_t g = 0; g < kAsmPerWave; ++g) {
        const uint32_t cg = uni32(__shfl(long_cnt, (int)(g * kAsmLanes), 64));
        if (cg == 0) continue;
        const uint64_t bg = uni64(__shfl(b, (int)(g * kAsmLanes), 64));
        assemble_large(A, s_large[wid], j0 + g, bg, cg, lane);
    }
}

static uint64_t n_tiles(uint64_t n) { return (n + kTileMsgs - 1) / kTileMsgs; }
static uint64_t n_groups(uint64_t n) { return (n + kGroupMsgs - 1) / kGroupMsgs; }

}  // namespace udpmsg
}  // namespace hyobfs

using namespace hyobfs;
using namespace hyobfs::udpmsg;

extern "C" {

int hyobfs_udp_parse_batch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint64_t n,
                           hyobfs_udp_parsed* out, void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!in || !in_off || !in_len || !out) return HYOBFS_ERR_INVALID;
    hipLaunchKernelGGL(udp_parse_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, in_off,
                       in_len, n, out);
    return hy_status(hipGetLastError());
}

uint64_t hyobfs_udp_frag_workspace_size(uint64_t n) { return (2 * (n_tiles(n) + 1) + n_groups(n)) * 8; }

int hyobfs_udp_frag_batch(const uint8_t* data, const uint64_t* data_off, const uint32_t* data_len,
                          const hyobfs_udp_meta* meta, const uint8_t* addrs, uint64_t n, uint8_t* out,
                          uint64_t out_cap, uint64_t* dgram_off, uint32_t* dgram_len, uint64_t dgram_cap,
                          uint64_t* first, int32_t* status, uint64_t* totals, void* workspace, void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!data || !data_off || !data_len || !meta || !addrs || !first || !status || !totals || !workspace ||
        (out_cap && !out) || (dgram_cap && (!dgram_off || !dgram_len)) || (reinterpret_cast<uintptr_t>(workspace) & 7))
        return HYOBFS_ERR_INVALID;
    const uint64_t ntiles = n_tiles(n);
    if (ntiles > 0x7FFFFFFFull) return HYOBFS_ERR_INVALID;
    uint64_t* const ws = static_cast<uint64_t*>(workspace);
    const FragArgs A{data,      data_off, data_len, meta,   addrs,  n,  out,          out_cap,           dgram_off,
                     dgram_len, dgram_cap, first,    status, totals, ws, ws + ntiles + 1, ws + 2 * (ntiles + 1)};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(udp_plan_kernel, dim3((uint32_t)ntiles), dim3(kTileMsgs), 0, s, A);
    hipLaunchKernelGGL(udp_scan_kernel, dim3(1), dim3(kScanTiles), 0, s, A.tile_bytes, A.tile_dgrams, ntiles);
    hipLaunchKernelGGL(udp_index_kernel, dim3((uint32_t)ntiles), dim3(kTileMsgs), 0, s, A);
    if (out_cap && dgram_cap)   // otherwise no message is written
        hipLaunchKernelGGL(udp_write_kernel, dim3((uint32_t)((n_groups(n) + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, s,
                           A);
    return hy_status(hipGetLastError());
}

int hyobfs_udp_assemble_batch(const uint8_t* in, const uint64_t* in_off, const hyobfs_udp_parsed* parsed, uint64_t n,
                              const uint32_t* frag_idx, const uint64_t* msg_first, uint64_t m, uint8_t* out,
                              const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len, int32_t* status,
                              void* stream) {
    if (m == 0) return HYOBFS_OK;
    if (!in || !in_off || !parsed || !frag_idx || !msg_first || !out || !out_off || !out_cap || !out_len || !status)
        return HYOBFS_ERR_INVALID;
    const uint64_t blocks = (m + kWaves * kAsmPerWave - 1) / (kWaves * kAsmPerWave);
    if (blocks > 0x7FFFFFFFull) return HYOBFS_ERR_INVALID;
    const AsmArgs A{in, in_off, parsed, n, frag_idx, msg_first, m, out, out_off, out_cap, out_len, status};
    hipLaunchKernelGGL(udp_assemble_kernel, dim3((uint32_t)blocks), dim3(64 * kWaves), 0, (hipStream_t)stream, A);
    return hy_status(hipGetLastError());
}

}  // extern "C"
