// sniff.hip -- TLS ClientHello server-name extraction for the sniffer
// (include/hyobfs_sniff.h).
//
// Reference: apernet/hysteria extras/sniff/sniff.go (isTLS :59-65, the TLS
// branch of TCP :128-144, UDP :159-174) and the ClientHello parse rules that
// the header states (Go's crypto/tls clientHelloMsg.unmarshal, which utls
// forks).
//
// One kernel, three front ends (a ClientHello message, the first bytes of a
// TCP stream, the CRYPTO data that quic_open_kernel assembled):
//   sni_kernel   one WAVE per message, four messages per 256-thread workgroup,
//                grid-stride over groups of four.  The parse is a serial walk
//                over length-prefixed fields of a message a few hundred bytes
//                long: the wave first stages the message (1 KiB of it at a
//                time) in LDS with coalesced loads that are all in flight
//                together, then walks it wave-uniform, every lane reading the
//                same LDS byte.  The types of the extensions seen
//                so far are a per-wave list in LDS, searched 64 entries per
//                step and a ballot.  The name is copied a byte per lane.
//   tcp_kernel   the first bytes of a TCP stream, by Sniffer.TCP's dispatch
//                (sniff.go:103-156), with the same shape: a wave looks at its
//                stream's first three bytes and runs the HTTP scan of
//                sniff_http.h or the record front end and the walk above.
//                With HTTP_ONLY it is the HTTP branch alone.
// Waves of a workgroup share nothing and never meet at a barrier, so a wave
// whose message fails at byte 0 does not wait for a neighbour's 256 extensions.
#include "kernels.h"
#include "../../include/hyobfs_sniff.h"
#include "sniff_http.h"

namespace hyobfs {
namespace sniff {

constexpr uint32_t kWaves = 4;          // messages per workgroup
// Workgroups per launch.  Far more than are resident at once (7 per CU at 72 VGPRs), so
// that the hardware dispatcher evens the load out: a grid of 2048 left 256 workgroups
// for a second round at low occupancy and took 1.2x as long.
constexpr uint32_t kGridCap = 1u << 16;
constexpr uint32_t kStage = 1024;       // bytes of a message a wave stages in LDS at a time

enum Mode { kHello = 0, kRecord = 1, kQuic = 2 };

struct SniArgs {
    const uint8_t* msgs;
    const uint64_t* off;
    const uint32_t* len;              // kHello / kRecord
    const hyobfs_quic_result* qres;   // kQuic: status and out_len of ReadCryptoPayload
    uint64_t n;
    uint8_t* names;
    uint32_t name_stride;
    hyobfs_sniff_result* res;
};

// wave-uniform byte reader over [0, n): the wave stages kStage bytes of its message in
// LDS with one round of independent, coalesced loads (a byte per lane each), then
// every lane reads the same LDS byte (a broadcast).  A message longer than kStage
// is staged again from the first byte the walk asks for past the staged part.
struct Window {
    const uint8_t* p;
    uint64_t n, base;
    uint8_t* lds;   // this wave's kStage bytes
    __device__ void fill(uint64_t at, uint32_t lane) {
        base = at;
        const uint64_t left = at < n ? n - at : 0;
        const uint32_t limit = left < kStage ? (uint32_t)left : kStage;
        uint8_t v[kStage / 64];
#pragma unroll
        for (uint32_t k = 0; k < kStage / 64; ++k) v[k] = lane + 64 * k < limit ? p[at + lane + 64 * k] : 0;
        hy_wave_sync();   // every lane's reads of the bytes staged before are done
#pragma unroll
        for (uint32_t k = 0; k < kStage / 64; ++k) lds[lane + 64 * k] = v[k];
        hy_wave_sync();
    }
    // bytes past n read as 0
    __device__ uint32_t u8(uint64_t i, uint32_t lane) {
        if (i < base || i >= base + kStage) fill(i, lane);
        return (uint32_t)__builtin_amdgcn_readfirstlane(lds[i - base]);
    }
    __device__ uint32_t u16(uint64_t i, uint32_t lane) {
        const uint32_t hi = u8(i, lane);
        return hi << 8 | u8(i + 1, lane);
    }
};

struct Parsed {
    int status;
    uint32_t name_off, name_len;
};

// The parse rules of include/hyobfs_sniff.h over w.p[start, end); `seen` is
// this wave's list of extension types.  Wave-uniform: every lane returns the
// same value.  name_off is relative to w.p.
__device__ Parsed parse_client_hello(Window& w, uint64_t start, uint64_t end, uint16_t* seen, uint32_t lane) {
    const Parsed bad{HYOBFS_SNIFF_ERR_MALFORMED, 0, 0};
    Parsed r{HYOBFS_OK, 0, 0};
    uint64_t i = start;
    if (end - i < 4 + 2 + 32 + 1) return bad;   // rules 1, 2 and the session_id length
    i += 4 + 2 + 32;
    const uint32_t sid = w.u8(i, lane);
    i += 1;
    if (end - i < sid) return bad;
    i += sid;
    if (end - i < 2) return bad;
    const uint32_t cs = w.u16(i, lane);
    i += 2;
    if (end - i < cs || (cs & 1)) return bad;
    i += cs;
    if (end - i < 1) return bad;
    const uint32_t cm = w.u8(i, lane);
    i += 1;
    if (end - i < cm) return bad;
    i += cm;
    if (i == end) return r;                      // rule 7: no extensions
    if (end - i < 2) return bad;
    const uint32_t el = w.u16(i, lane);
    i += 2;
    if (end - i != el) return bad;               // rule 8
    uint32_t cnt = 0;
    bool have = false;
    while (i < end) {
        if (end - i < 4) return bad;             // rule 9
        const uint32_t typ = w.u16(i, lane), bl = w.u16(i + 2, lane);
        i += 4;
        if (end - i < bl) return bad;
        if (cnt == HYOBFS_TLS_MAX_EXTENSIONS) return Parsed{HYOBFS_SNIFF_ERR_EXTENSIONS, 0, 0};
        bool dup = false;                        // rule 10
        for (uint32_t k = lane; k < cnt; k += 64) dup |= seen[k] == typ;
        if (__ballot(dup)) return bad;
        if (lane == 0) seen[cnt] = (uint16_t)typ;
        ++cnt;
        hy_wave_sync();   // lane 0's entry is visible to the next search
        if (typ == 0) {                          // rule 11
            if (bl < 2) return bad;
            const uint32_t ll = w.u16(i, lane);
            if (ll == 0 || ll + 2 != bl) return bad;
            uint64_t j = i + 2;
            const uint64_t le = j + ll;
            while (j < le) {
                if (le - j < 3) return bad;
                const uint32_t nt = w.u8(j, lane), nl = w.u16(j + 1, lane);
                j += 3;
                if (le - j < nl || nl == 0) return bad;
                if (nt == 0) {
                    if (have) return bad;
                    have = true;
                    r.name_off = (uint32_t)j;
                    r.name_len = nl;
                    if (w.u8(j + nl - 1, lane) == '.') return bad;
                }
                j += nl;
            }
        }
        i += bl;
    }
    return r;
}

template <int MODE>
__global__ __launch_bounds__(64 * kWaves) void sni_kernel(SniArgs a) {
    __shared__ uint16_t seen_all[kWaves][HYOBFS_TLS_MAX_EXTENSIONS];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ uint8_t stage_all[kWaves][kStage];
    uint16_t* seen = seen_all[wave];
    for (uint64_t m = (uint64_t)blockIdx.x * kWaves + wave; m < a.n; m += (uint64_t)gridDim.x * kWaves) {
        hyobfs_sniff_result out{};
        uint64_t L;
        if (MODE == kQuic) {
            const hyobfs_quic_result q = a.qres[m];
            if (q.status != HYOBFS_OK) {         // nothing is read from a failed packet's slot
                out.status = HYOBFS_SNIFF_ERR_NO_PAYLOAD;
                if (lane == 0) a.res[m] = out;
                continue;
            }
            L = q.out_len;
        } else {
            L = a.len[m];
        }
        const uint8_t* p = a.msgs + a.off[m];
        Window w{p, L, 0, stage_all[wave]};
        w.fill(0, lane);
        uint64_t start = 0, end = L;
        int st = HYOBFS_OK;
        if (MODE == kRecord) {
            // isTLS (sniff.go:59-65), then the record length (sniff.go:128-143)
            const uint32_t b0 = w.u8(0, lane), b1 = w.u8(1, lane), b2 = w.u8(2, lane);   // zero past L
            if (L < 3 || b0 < 0x16 || b0 > 0x17 || b1 != 0x03 || b2 > 0x09) {
                st = HYOBFS_SNIFF_ERR_NOT_TLS;
            } else {
                const uint64_t need = L < 5 ? 5 : 5 + (uint64_t)w.u16(3, lane);
                if (L < need) {
                    st = HYOBFS_SNIFF_ERR_NEED_MORE;
                    out.need = (uint32_t)need;
                }
                start = 5;
                end = need;
            }
        } else if (L < 4 || w.u8(0, lane) != 0x01) {   // sniff.go:161
            st = HYOBFS_SNIFF_ERR_NOT_HELLO;
        }
        if (st == HYOBFS_OK) {
            const Parsed r = parse_client_hello(w, start, end, seen, lane);
            st = r.status;
            if (st == HYOBFS_OK && r.name_len) {
                out.name_len = r.name_len;
                out.name_off = r.name_off;
                if (r.name_len > a.name_stride) {
                    st = HYOBFS_SNIFF_ERR_NAME_CAP;
                } else {
                    uint8_t* d = a.names + m * a.name_stride;
                    const uint8_t* s = p + r.name_off;
                    for (uint32_t q = lane; q < r.name_len; q += 64) d[q] = s[q];
                }
            }
        }
        out.status = st;
        if (lane == 0) a.res[m] = out;
    }
}

// Sniffer.TCP over the first bytes of a stream: isHTTP, else isTLS, else
// unrecognised (HTTP_ONLY: the HTTP branch alone, NOT_HTTP otherwise).
template <bool HTTP_ONLY>
__global__ __launch_bounds__(64 * kWaves) void tcp_kernel(SniArgs a) {
    __shared__ uint16_t seen_all[kWaves][HTTP_ONLY ? 1 : HYOBFS_TLS_MAX_EXTENSIONS];
    static_assert(kStage >= kHttpStage, "the HTTP scan stages in the same LDS bytes");
    __shared__ uint8_t stage_all[kWaves][kStage];
    // the wave's number as a scalar, so that m, the stream's length and address and every loop over them are scalar
    const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t m = (uint64_t)blockIdx.x * kWaves + wave; m < a.n; m += (uint64_t)gridDim.x * kWaves) {
        const uint32_t L = a.len[m];
        const uint8_t* p = a.msgs + a.off[m];
        HttpParsed r = http_parse(p, L, stage_all[wave], lane);
        if (!HTTP_ONLY && r.status == HYOBFS_SNIFF_ERR_NOT_HTTP) {
            if (L < 3) {
                r = HttpParsed{HYOBFS_SNIFF_ERR_NEED_MORE, 0, 0, 3};
            } else if (uni(p[0]) < 0x16 || uni(p[0]) > 0x17 || uni(p[1]) != 0x03 || uni(p[2]) > 0x09) {   // isTLS, :59-65
                r.status = HYOBFS_SNIFF_ERR_UNRECOGNIZED;
            } else {                                                                  // sniff.go:128-143
                Window w{p, L, 0, stage_all[wave]};
                w.fill(0, lane);
                const uint32_t need = L < 5 ? 5 : 5 + w.u16(3, lane);
                if (L < need) {
                    r = HttpParsed{HYOBFS_SNIFF_ERR_NEED_MORE, 0, 0, need};
                } else {
                    const Parsed t = parse_client_hello(w, 5, need, seen_all[wave], lane);
                    r = HttpParsed{t.status, t.name_off, t.name_len, 0};   // both 0 unless OK
                }
            }
        }
        hyobfs_sniff_result out{r.status, r.name_len, r.name_off, r.need};
        if (r.status == HYOBFS_OK && r.name_len) {
            if (r.name_len > a.name_stride) {
                out.status = HYOBFS_SNIFF_ERR_NAME_CAP;
            } else {
                uint8_t* d = a.names + m * a.name_stride;
                const uint8_t* s = p + r.name_off;
                for (uint32_t q = lane; q < r.name_len; q += 64) d[q] = s[q];
            }
        }
        if (lane == 0) a.res[m] = out;
    }
}

inline uint32_t grid_for(uint64_t n) {
    const uint64_t g = (n + kWaves - 1) / kWaves;
    return (uint32_t)(g < kGridCap ? g : kGridCap);
}

template <int MODE>
inline int launch(const SniArgs& a, void* stream) {
    hipLaunchKernelGGL(sni_kernel<MODE>, dim3(grid_for(a.n)), dim3(64 * kWaves), 0, static_cast<hipStream_t>(stream),
                       a);
    return hy_status(hipGetLastError());
}

template <bool HTTP_ONLY>
inline int launch_tcp(const SniArgs& a, void* stream) {
    hipLaunchKernelGGL(tcp_kernel<HTTP_ONLY>, dim3(grid_for(a.n)), dim3(64 * kWaves), 0,
                       static_cast<hipStream_t>(stream), a);
    return hy_status(hipGetLastError());
}

static_assert(sizeof(hyobfs_sniff_result) == 16, "hyobfs_sniff_result layout");

}  // namespace sniff
}  // namespace hyobfs

using namespace hyobfs::sniff;

extern "C" {

int hyobfs_tls_client_hello_sni_batch(const uint8_t* msgs, const uint64_t* off, const uint32_t* len, uint64_t n,
                                      uint8_t* names, uint32_t name_stride, hyobfs_sniff_result* res,
                                      void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!msgs || !off || !len || !names || !res) return HYOBFS_ERR_INVALID;
    return launch<kHello>(SniArgs{msgs, off, len, nullptr, n, names, name_stride, res}, stream);
}

int hyobfs_tls_record_sni_batch(const uint8_t* msgs, const uint64_t* off, const uint32_t* len, uint64_t n,
                                uint8_t* names, uint32_t name_stride, hyobfs_sniff_result* res, void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!msgs || !off || !len || !names || !res) return HYOBFS_ERR_INVALID;
    return launch<kRecord>(SniArgs{msgs, off, len, nullptr, n, names, name_stride, res}, stream);
}

int hyobfs_http_request_host_batch(const uint8_t* msgs, const uint64_t* off, const uint32_t* len, uint64_t n,
                                   uint8_t* names, uint32_t name_stride, hyobfs_sniff_result* res, void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!msgs || !off || !len || !names || !res) return HYOBFS_ERR_INVALID;
    return launch_tcp<true>(SniArgs{msgs, off, len, nullptr, n, names, name_stride, res}, stream);
}

int hyobfs_tcp_sniff_batch(const uint8_t* msgs, const uint64_t* off, const uint32_t* len, uint64_t n, uint8_t* names,
                           uint32_t name_stride, hyobfs_sniff_result* res, void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!msgs || !off || !len || !names || !res) return HYOBFS_ERR_INVALID;
    return launch_tcp<false>(SniArgs{msgs, off, len, nullptr, n, names, name_stride, res}, stream);
}

uint64_t hyobfs_quic_sniff_workspace_size(uint64_t n) { return hyobfs_quic_workspace_size(n); }

int hyobfs_quic_sniff_batch(uint8_t* packets, const uint64_t* off, const uint32_t* len, uint64_t n, uint8_t* crypto,
                            const uint64_t* crypto_off, const uint32_t* crypto_cap, hyobfs_quic_result* qres,
                            uint8_t* names, uint32_t name_stride, hyobfs_sniff_result* sres, void* workspace,
                            void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!names || !sres) return HYOBFS_ERR_INVALID;
    const int rc = hyobfs_quic_read_crypto_payload_batch(packets, off, len, n, crypto, crypto_off, crypto_cap, qres,
                                                         workspace, stream);
    if (rc != HYOBFS_OK) return rc;
    return launch<kQuic>(SniArgs{crypto, crypto_off, nullptr, qres, n, names, name_stride, sres}, stream);
}

}  // extern "C"
