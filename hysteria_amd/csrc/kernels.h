// Private interface between the C ABI layer (hyobfs_api.cpp) and the gfx950
// kernels (salamander.hip).  Not installed; include/hyobfs.h is the ABI.
#pragma once
#ifdef HYOBFS_EMULATE
#include "hip_emu.h"   // tests/emu: CPU emulation for the CPU test tier, never shipped
#else
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "../../include/hyobfs.h"
#include "../../include/hyobfs_gecko.h"

// small functions shared by host and device code (sha256.h, quic_crypto.h)
#define HY_HD __host__ __device__ __forceinline__

namespace hyobfs {

// the C ABI's status for the result of a HIP call or launch
inline int hy_status(hipError_t e) { return e == hipSuccess ? HYOBFS_OK : HYOBFS_ERR_HIP; }

// Orders one wave's LDS writes before its later LDS reads by other lanes of the
// same wave.  A wave's LDS instructions execute in order, so this only has to
// stop the compiler from moving memory operations across it (wavefront-scope
// fences emit no instruction).
#ifdef HYOBFS_EMULATE
inline void hy_wave_sync() { hyemu_wave_sync(); }
#else
__device__ __forceinline__ void hy_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
#endif

constexpr int kTile = 256;          // datagrams per tile-sum entry of the packed layout's scan
constexpr uint32_t kMaxDatagram = HYOBFS_BATCH_MAX_DATAGRAM;   // longest datagram a call accepts (include/hyobfs.h)
static_assert(kMaxDatagram == (1u << 24) - 64, "the wave kernel's 32-bit virtual offsets assume 64 datagrams < 2^30");
constexpr uint64_t kMaxStride = 1ull << 24;         // longest slot of a slotted output
// batch kernels (include/hyobfs.h HYOBFS_KERNEL_*)
constexpr int kKernelAuto = 0, kKernelWave = 1, kKernelTile = 2, kKernelFlat = 3;

// BLAKE2b state for the per-packet key, precomputed on the host from the PSK
// alone (salamander.go:88-91 hashes PSK || salt; every block before the one
// holding salt[0] depends on the PSK only).  The device compresses the last
// one or two blocks, which carry the salt.
struct KeyParams {
    uint64_t h[8];       // chaining value entering the first device block
    uint64_t m[32];      // message words of the device blocks, salt bytes = 0
    uint64_t t[2];       // byte counter after each device block
    uint32_t nblk;       // 1 or 2 device blocks
    uint32_t salt_pos;   // byte offset of salt[0] in the device blocks (0..127)
};

// The kernels that hash a salt are instantiated once per salt word SW = salt_pos / 8
// (0..15): the PSK's message words stay scalar, only the salt's one or two words are per
// lane.  Calls f(std::integral_constant<int, SW>) and returns its result;
// hipErrorInvalidValue for a salt_pos of 128 or more (unreachable: make_key_params).
template <class F, int... SW>
hipError_t with_salt_word(uint32_t sw, F&& f, std::integer_sequence<int, SW...>) {
    hipError_t e = hipErrorInvalidValue;
    (void)(... || (sw == SW && ((e = f(std::integral_constant<int, SW>{})), true)));
    return e;
}
template <class F>
hipError_t with_salt_word(const KeyParams& k, F&& f) {
    return with_salt_word(k.salt_pos >> 3, f, std::make_integer_sequence<int, 16>{});
}

// One batch launch: the kernels' argument.  The caller of launch_salamander fills the
// fields of include/hyobfs.h's struct hyobfs_batch, `kernel` and the one scratch pointer;
// the derived fields (tile_prefix, tile_sums, in_tile_sums, in_tile_prefix, run_log2,
// blk0) are written by the launchers only, on their own copy.
struct BatchParams {
    uint64_t n;
    const uint8_t* in;
    const uint64_t* in_off;
    uint64_t in_stride;
    const uint32_t* in_len;
    uint32_t len_uniform;
    uint32_t pkt_cap;       // effective per-packet cap (slot and pkt_cap folded), 0 = none
    const uint64_t* salts;
    uint8_t* out;
    uint64_t out_cap;
    uint64_t out_stride;    // 0 = packed
    uint64_t* out_off;
    uint32_t* out_len;
    unsigned long long* out_total;
    const uint64_t* tile_prefix;  // packed: exclusive prefix of tile sums (ntiles+1)
    uint64_t* tile_sums;          // packed: scratch, ntiles+1 entries
    // contiguous input, packed output on the wave kernel: per-tile sums of the input
    // lengths (scratch, ntiles+1) and their exclusive prefix (the input offsets)
    uint64_t* in_tile_sums = nullptr;
    const uint64_t* in_tile_prefix = nullptr;
    void* scratch;                // device scratch of BatchPlan::scratch_bytes bytes (unused when that is 0)
    uint32_t run_log2;            // wave kernel: datagrams per run = 2^run_log2
    uint64_t blk0 = 0;            // wave kernel, packed runs of 64: first workgroup of this launch
    int kernel;                   // HYOBFS_KERNEL_* of the context (0 = auto)
};

struct TileParams {   // the tile kernel's view of a batch (salamander_tile.h, tile_params)
    uint32_t S;      // output slot (out_stride), a multiple of 8
    uint32_t W;      // output width, a multiple of 8, 16 <= W <= S
    uint32_t LI;     // input bytes per datagram (len_uniform)
    float invS;      // 1 / S
    uint64_t t0;     // first tile of this launch (launch_tile_sw splits big batches)
};

// What launch_salamander issues in front of the main kernel.  ntiles = ceil(n / kTile).
enum class Prepass {
    kNone,          // slotted output, explicit or strided input
    kWidthScan,     // packed output, explicit or strided input: the width sums and their scan
    kPackedScans,   // contiguous input into packed output, runs of 64: width and length sums, scanned in one launch
    kInputOffsets,  // contiguous input into slots or shortened packed runs: length sums, their scan, the input
                    // offsets; then an explicit-offset batch (packed: with kWidthScan's launches)
    kFlatLocate,    // the flat kernel's: both sums, both scans, flat_locate_kernel
};

// The host's whole answer for one batch: which kernel runs, what runs in front of it, and
// how the one scratch allocation is laid out.  plan_batch decides it; the workspace
// query, the kernel query and launch_salamander only read it.
struct BatchPlan {
    int kernel;             // kKernelTile / kKernelWave / kKernelFlat; kKernelAuto: n == 0, nothing runs
    Prepass prepass;
    TileParams tile;        // kernel == kKernelTile
    // byte offsets into BatchParams::scratch (a region the prepass does not use has no room there)
    uint64_t width_sums;    // ntiles + 1 words
    uint64_t len_sums;      // ntiles + 1 words
    uint64_t in_off;        // kInputOffsets: n words
    uint64_t flat_cut;      // kFlatLocate: the two cut words
    uint64_t flat_desc;     // kFlatLocate: the tile descriptors (with the cut words flat_desc_bytes)
    uint64_t flat_krec;     // kFlatLocate: the key records start at the next address that is a multiple of 256
    uint64_t scratch_bytes; // the whole allocation (0: none)
};
// Pure (no device call): reads the batch and the process-wide knobs (HYOBFS_KERNEL,
// HYOBFS_PACKED_RUN_LOG2), each of them read once per process.
BatchPlan plan_batch(bool obfuscate, const BatchParams& b);

// HYOBFS_KERNEL_* that a context's setting resolves to (AUTO: the
// HYOBFS_KERNEL environment variable, else 0)
int resolve_kernel(int ctx_kernel);
// runs plan = plan_batch(obfuscate, b) on b; b.scratch holds plan.scratch_bytes bytes
hipError_t launch_salamander(bool obfuscate, const BatchPlan& plan, const BatchParams& b, const KeyParams& k,
                             hipStream_t s);
// contiguous input: datagram i at in + in_len[0] + ... + in_len[i-1]
inline bool contiguous_input(const BatchParams& b) { return !b.in_off && b.in_stride == 0 && b.in_len && b.n > 1; }
hipError_t launch_keys(const KeyParams& k, const uint64_t* salts, uint8_t* keys, uint64_t n,
                       hipStream_t s);
hipError_t launch_gecko_encode(const KeyParams& k, const hyobfs_gecko_batch& b, hipStream_t s);
hipError_t launch_gecko_parse(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint64_t n,
                              hyobfs_gecko_parsed* out, hipStream_t s);
// hyobfs_gecko_peek_batch / hyobfs_gecko_open_batch (include/hyobfs_gecko.h); hipErrorInvalidValue: a batch
// too large for one grid
hipError_t launch_gecko_peek(const KeyParams& k, const uint8_t* wire, const uint64_t* wire_off, const uint32_t* wire_len,
                             uint64_t n, hyobfs_gecko_parsed* parsed, uint8_t* keys, hipStream_t s);
struct GeckoOpenArgs {
    const uint8_t* wire;
    const uint64_t* wire_off;
    const uint32_t* wire_len;
    const hyobfs_gecko_parsed* parsed;
    const uint8_t* keys;
    uint64_t n;
    const uint32_t* chunk_idx;
    const uint64_t* msg_first;
    uint64_t m;
    uint8_t* out;
    const uint64_t* out_off;
    const uint32_t* out_cap;
    uint32_t* out_len;
    int32_t* status;
};
hipError_t launch_gecko_open(const GeckoOpenArgs& a, hipStream_t s);
hipError_t launch_synth_stream(uint8_t* dst, uint64_t nbytes, uint64_t seed, uint64_t start,
                               hipStream_t s);
hipError_t launch_synth_u64(uint64_t* dst, uint64_t n, uint64_t seed, uint64_t first,
                            hipStream_t s);
hipError_t launch_synth_bimodal(uint32_t* dst, uint64_t n, uint64_t seed, uint64_t first,
                                hipStream_t s);

}  // namespace hyobfs
