"""The limits lattice of the Salamander batch kernels (hysteria_amd/csrc/salamander_tile.h,
salamander_wave.h, salamander_flat.h, the dispatch in salamander.hip and fill_params in
hyobfs_api.cpp), shared by the CPU tier (tests/test_batch_limits.py through
tests/emu/batch_main.cpp) and the GPU tier (tests/test_gpu_batch_limits.py).

Every case is built from the oracles alone (oracle/salamander_ref.py: hashlib's BLAKE2b
and the batch rules of include/hyobfs.h restated in Python); this module never imports
the product package.  A case is a dict:

  name, family, obf, psk, n
  inp (uint8 array of exactly the bytes the header promises), in_align (0 or 8: the
  input base modulo 16), in_off / in_len (arrays or None), in_stride, len_uniform
  salts (uint64, obfuscate), out_cap, out_stride, pkt_cap
  settings: [(kernel setting, what hyobfs_salamander_batch_kernel must answer)], the
            answer a kernel name or INVALID
  status, out_off, out_len, out_total, regions [(offset, bytes)]: the expected results;
            every byte of `out` outside the regions keeps the caller's fill

Families (NAMES[family] lists the case names, build(name) makes one):

  slot_estimate   slots at which the tile kernel's float32 estimate of a chunk's datagram,
                  p = (uint32)((float)x * (1.0f / S)), is one too low, so its `r >= S`
                  repair runs: S = 328, 376, 656 dense and gapped, full, one-datagram and
                  partial tiles, and one slot just under 2^20.
  length_ladder   datagram lengths from 4096 up to 2^32 - 1 around the library's limit
                  M = HYOBFS_BATCH_MAX_DATAGRAM, as uniform slots, in ragged packed batches
                  next to ordinary datagrams, and as contiguous input.
  eligibility     one pair of cases per predicate of tile_params / fill_params, differing
                  in that predicate only (PAIRS).
  input_aliasing  input layouts in which datagrams share bytes: broadcast (stride 0),
                  overlapping windows (stride 8), equal and descending offsets.
"""
import struct

import numpy as np

from oracle import salamander_ref as ref

M = ref.BATCH_MAX_DATAGRAM
PSK = b"average_password"
INVALID = -2                      # HYOBFS_ERR_INVALID
SENTINEL = 0xA5
UNSET = 0xEE                      # fill of out_off / out_len / out_total before a call
SETTING_ID = {"auto": 0, "wave": 1, "tile": 2, "flat": 3}      # HYOBFS_KERNEL_*
KERNEL_ID = {"none": 0, "wave": 1, "tile": 2, "flat": 3}
MAX_TILE_SLOT = 1 << 20
TILE = 16                         # datagrams per tile

LADDER = [4096, 4097, 4104, 9000, 65507, 65535, 65536, 65544, 1 << 20, M - 8, M, M + 1, M + 8, 1 << 24,
          0xFFFFFFF7, 0xFFFFFFF8, 0xFFFFFFFF]
LOW_SLOTS = [328, 376, 656]
LARGE_LOW_SLOT = 1048360


# ------------------------------------------------------------------ the tile kernel's slot estimate
def slot_estimate(S, x):
    """The datagram the tile kernel first assigns to the chunks at tile-local byte
    offsets x (uint32 array): the product of two float32 values, truncated."""
    inv = np.float32(1.0) / np.float32(S)
    prod = x.astype(np.float32) * inv
    assert prod.dtype == np.float32
    return prod.astype(np.uint32)


def estimate_errors(S, x):
    """(low, high) masks over x: the estimate is below / above x // S."""
    x = np.asarray(x, np.uint32)
    est = slot_estimate(S, x).astype(np.int64)
    true = x.astype(np.int64) // S
    return est < true, est > true


def low_chunks(S, nt, W):
    """Chunks of a tile of nt datagrams whose estimate is low and whose low half is a
    written byte (so a kernel without the repair writes something else there)."""
    x = np.arange(0, (nt - 1) * S + W, 16, dtype=np.uint32)
    low, _ = estimate_errors(S, x)
    r = x.astype(np.int64) % S
    return x[low & (r < W)]


def sweep_slot_estimates():
    """The restatement over every eligible slot (multiples of 8 from 16 to 2^20): every
    chunk of a full tile for S <= 2^14, the chunks next to each multiple of S above.
    Returns (number of slots with a low estimate, number with a high one)."""
    low_slots = high_slots = 0
    for S in range(16, (1 << 14) + 1, 8):
        low, high = estimate_errors(S, np.arange(0, TILE * S, 16, dtype=np.uint32))
        low_slots += bool(low.any())
        high_slots += bool(high.any())
    S = np.arange((1 << 14) + 8, MAX_TILE_SLOT + 1, 8, dtype=np.int64)
    k = np.arange(1, TILE, dtype=np.int64)
    base = (S[:, None] * k[None, :]) // 16 * 16                      # the chunk holding byte k S
    x = (base[:, :, None] + np.array([-16, 0, 16], np.int64)[None, None, :]).astype(np.uint32)
    inv = (np.float32(1.0) / S.astype(np.float32))[:, None, None]
    est = (x.astype(np.float32) * inv).astype(np.uint32).astype(np.int64)
    true = x.astype(np.int64) // S[:, None, None]
    low_slots += int((est < true).any(axis=(1, 2)).sum())
    high_slots += int((est > true).any(axis=(1, 2)).sum())
    return low_slots, high_slots


# ------------------------------------------------------------------ the kernel AUTO / WAVE / FLAT must report
def _cap(cs):
    cap = cs["pkt_cap"]
    if cs["out_stride"] and (cap == 0 or cs["out_stride"] < cap):
        cap = cs["out_stride"]
    return cap


def contiguous(cs):
    return cs["in_off"] is None and cs["in_stride"] == 0 and cs["in_len"] is not None and cs["n"] > 1


def tile_eligible(cs):
    """include/hyobfs.h: "slotted batches whose region edges are all multiples of 8 (one
    length, slot and input stride multiples of 8, payloads of 16 bytes or more, nothing
    dropped)", with the limits DESIGN.md gives the tile kernel: 16-byte aligned input,
    datagrams and input strides of at most 4096 bytes, slots of at most 2^20."""
    L, S, n = cs["len_uniform"], cs["out_stride"], cs["n"]
    if S == 0 or cs["in_len"] is not None or cs["in_off"] is not None or n == 0:
        return False
    W = L + 8 if cs["obf"] else L - 8
    return (L <= M and L >= (16 if cs["obf"] else 24) and (L | S | cs["in_stride"] | cs["in_align"]) % 8 == 0
            and cs["in_align"] % 16 == 0 and cs["in_stride"] <= 4096 and L <= 4096
            and (_cap(cs) == 0 or W <= _cap(cs)) and W <= S and (n - 1) * S + W <= cs["out_cap"]
            and S <= MAX_TILE_SLOT)


def kernel_for(cs, setting):
    if cs["out_stride"] > M:
        return INVALID
    if cs["n"] == 0:
        return "none"
    if setting == "flat" and contiguous(cs) and cs["out_stride"] == 0 and cs["in_align"] % 16 == 0:
        return "flat"
    if setting == "wave":
        return "wave"
    return "tile" if tile_eligible(cs) else "wave"


# ------------------------------------------------------------------ building blocks
def _bytes(seed, n):
    return np.frombuffer(ref.stream_bytes(seed, 0, n), np.uint8).copy()


def _wire(psk, seed, L, salt):
    """A real wire datagram of L bytes (L > 8), or L arbitrary bytes (dropped on deobfuscate)."""
    if L <= 8:
        return _bytes(seed, L)
    return np.frombuffer(ref.obfuscate(psk, ref.stream_bytes(seed, 0, L - 8), int(salt).to_bytes(8, "little")), np.uint8)


def _finish(cs, settings, expect=None):
    """Adds the expected results (the oracle's) and the expected kernels."""
    cs.setdefault("psk", PSK)
    cs.setdefault("in_align", 0)
    cs.setdefault("pkt_cap", 0)
    n = cs["n"]
    if cs.get("salts") is None:
        cs["salts"] = ref.splitmix64_array(2, 7, n)
    cs["settings"] = [(s, kernel_for(cs, s)) for s in settings]
    if expect is not None:     # the eligibility cases state AUTO's answer themselves
        assert dict(cs["settings"])["auto"] == expect, (cs["name"], cs["settings"], expect)
        if "wave" in dict(cs["settings"]) and expect != INVALID:
            assert dict(cs["settings"])["wave"] == "wave"
    if cs["out_stride"] > M:
        cs["status"] = INVALID
        cs["regions"] = []
        cs["out_off"] = np.full(n, int.from_bytes(bytes([UNSET]) * 8, "little"), np.uint64)
        cs["out_len"] = np.full(n, int.from_bytes(bytes([UNSET]) * 4, "little"), np.uint32)
        cs["out_total"] = int.from_bytes(bytes([UNSET]) * 8, "little")
        return cs
    cs["status"] = 0
    cs["regions"], cs["out_off"], cs["out_len"], cs["out_total"] = ref.batch(
        cs["obf"], cs["psk"], n, cs["inp"], in_off=cs["in_off"], in_stride=cs["in_stride"], in_len=cs["in_len"],
        len_uniform=cs["len_uniform"], salts=cs["salts"], out_cap=cs["out_cap"], out_stride=cs["out_stride"],
        pkt_cap=cs["pkt_cap"])
    return cs


def _uniform(name, family, obf, n, L, S, *, in_stride=None, out_cap=None, settings=("auto", "wave"), expect=None,
             psk=PSK, seed=1, **kw):
    """n datagrams of L bytes at a stride of in_stride (default L) into slots of S bytes
    (0: packed); the input ends at the last datagram's last byte.  Deobfuscate input is real
    wire where the datagrams do not overlap.  Over-limit lengths get 16 bytes of input
    (none of it may be read)."""
    in_stride = L if in_stride is None else in_stride
    salts = ref.splitmix64_array(2, seed, n)
    if L > M:
        inp = _bytes(seed, 16)
    elif obf or in_stride < L:
        inp = _bytes(seed, (n - 1) * in_stride + L)
    else:
        inp = np.zeros((n - 1) * in_stride + L, np.uint8)
        inp[:] = 0x5A
        for i in range(n):
            inp[i * in_stride:i * in_stride + L] = _wire(psk, seed + i, L, salts[i])
    W = L + 8 if obf else L - 8
    if out_cap is None:
        out_cap = (n * S if S else n * max(W, 0)) + 16
    cs = dict(name=name, family=family, obf=obf, psk=psk, n=n, inp=inp, in_off=None, in_len=None, in_stride=in_stride,
              len_uniform=L, salts=salts, out_cap=out_cap, out_stride=S, **kw)
    return _finish(cs, settings, expect)


def _ragged(name, obf, special, seed, contig, settings):
    """About 70 datagrams of 0..2100 bytes with the lengths `special` spread among them,
    into packed output.  Explicit offsets: gaps of 0..3 bytes, a datagram over the limit
    points at the end of the buffer.  Contiguous: back to back, the one over-limit length
    (at most one) last."""
    rng = np.random.default_rng(seed)
    lens = [int(x) for x in rng.integers(0, 2101, 70)]
    lens[:4] = [0, 8, 9, 16]
    over = [s for s in special if s > M]
    for j, s in enumerate(s for s in special if s <= M):
        lens.insert(min(len(lens), 5 + 7 * j), s)        # a giant between tiny neighbours, several per group of 64
    if contig:
        assert len(over) <= 1
        lens += over
    else:
        for j, s in enumerate(over):
            lens.insert(11 + 9 * j, s)                    # datagrams after a dropped one show whether offsets moved
    n = len(lens)
    salts = ref.splitmix64_array(2, seed, n)
    parts, off, pos = [], np.zeros(n, np.uint64), 0
    for i, L in enumerate(lens):
        if L > M:
            off[i] = 0          # patched below: the end of the buffer
            continue
        if not contig:
            gap = int(rng.integers(0, 4))
            parts.append(np.full(gap, 0x3C, np.uint8))
            pos += gap
        off[i] = pos
        parts.append(_bytes(seed * 1000 + i, L) if obf else _wire(PSK, seed * 1000 + i, L, salts[i]))
        pos += L
    inp = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    for i, L in enumerate(lens):
        if L > M:
            off[i] = len(inp)
    in_len = np.array(lens, np.uint32)
    total = sum((L + 8 if obf else max(L - 8, 0)) for L in lens if L <= M)
    cs = dict(name=name, family="length_ladder", obf=obf, n=n, inp=inp, in_off=None if contig else off, in_len=in_len,
              in_stride=0, len_uniform=0, salts=salts, out_cap=total + 24, out_stride=0)
    if contig:      # the oracle reads contiguous input by the same rule; check it against the layout built here
        assert int(in_len[in_len <= M].astype(np.uint64).sum()) == len(inp)
    return _finish(cs, settings)


# ------------------------------------------------------------------ the families
REGISTRY = {}        # name -> (family, builder)
NAMES = {"slot_estimate": [], "length_ladder": [], "eligibility": [], "input_aliasing": []}
PAIRS = []           # eligibility: (case, case, what differs: "kernel" / "drops" / "status")
EXPECT_AUTO = {}     # eligibility: the kernel AUTO must report, stated case by case


def _reg(family, name, fn):
    assert name not in REGISTRY
    REGISTRY[name] = (family, fn)
    NAMES[family].append(name)


def _r8(x):
    return (x + 7) // 8 * 8


def _register():
    # ---- slot_estimate
    for S in LOW_SLOTS:
        for n in (16, 17, 33):
            _reg("slot_estimate", "est_S%d_n%d_dense_obf" % (S, n),
                 lambda S=S, n=n: _uniform("est_S%d_n%d_dense_obf" % (S, n), "slot_estimate", True, n, S - 8, S, seed=S + n))
            _reg("slot_estimate", "est_S%d_n%d_dense_deobf" % (S, n),
                 lambda S=S, n=n: _uniform("est_S%d_n%d_dense_deobf" % (S, n), "slot_estimate", False, n, S + 8, S, seed=S + n))
            _reg("slot_estimate", "est_S%d_n%d_gapped_obf" % (S, n),
                 lambda S=S, n=n: _uniform("est_S%d_n%d_gapped_obf" % (S, n), "slot_estimate", True, n, 96, S, seed=S + n))
    _reg("slot_estimate", "est_S%d_n17_obf" % LARGE_LOW_SLOT,
         lambda: _uniform("est_S%d_n17_obf" % LARGE_LOW_SLOT, "slot_estimate", True, 17, 96, LARGE_LOW_SLOT, seed=5))

    # ---- length_ladder: uniform slots
    for L in LADDER:
        for obf in (True, False):
            W = L + 8 if obf else L - 8
            n = 3 if L <= (1 << 20) or L > M else 2
            S = 4096 if L > M else min(_r8(W) + 8, M)       # over the limit: any valid slot, all dropped
            nm = "ladder_uniform_%s_L%d" % ("obf" if obf else "deobf", L)
            _reg("length_ladder", nm, lambda nm=nm, obf=obf, n=n, L=L, S=S: _uniform(nm, "length_ladder", obf, n, L, S,
                                                                                     seed=L % 1000))
    # ---- length_ladder: ragged packed with explicit offsets, and contiguous input
    rag_a = [4096, 4097, 9000, 65507, 65536, 1 << 20, M - 8, M + 8, 1 << 24, 0xFFFFFFF7, 0xFFFFFFFF]
    rag_b = [4104, 65535, 65544, M, M + 1, 0xFFFFFFF8]
    assert sorted(rag_a + rag_b) == sorted(LADDER)
    for obf in (True, False):
        d = "obf" if obf else "deobf"
        _reg("length_ladder", "ladder_ragged_a_" + d, lambda obf=obf, d=d: _ragged("ladder_ragged_a_" + d, obf, rag_a, 31,
                                                                                 False, ("auto", "wave")))
        _reg("length_ladder", "ladder_ragged_b_" + d, lambda obf=obf, d=d: _ragged("ladder_ragged_b_" + d, obf, rag_b, 32,
                                                                                 False, ("auto", "wave")))
        small = [4096, 4097, 4104, 9000, 65507, 65535, 65536, 65544, 1 << 20]
        _reg("length_ladder", "ladder_contig_a_" + d, lambda obf=obf, d=d: _ragged(
            "ladder_contig_a_" + d, obf, small + [M - 8, M + 8], 33, True, ("auto", "wave", "flat")))
        _reg("length_ladder", "ladder_contig_b_" + d, lambda obf=obf, d=d: _ragged(
            "ladder_contig_b_" + d, obf, [4096, 65536, M, M + 1], 34, True, ("auto", "wave", "flat")))
        for j, last in enumerate([1 << 24, 0xFFFFFFF7, 0xFFFFFFF8, 0xFFFFFFFF]):
            nm = "ladder_contig_last%x_%s" % (last, d)
            _reg("length_ladder", nm, lambda nm=nm, obf=obf, last=last, j=j: _ragged(
                nm, obf, [4097, 65535, last], 35 + j, True, ("auto", "wave", "flat")))

    # ---- eligibility
    def el(name, expect, fn):
        EXPECT_AUTO[name] = expect
        _reg("eligibility", name, lambda: fn(name, expect))

    def u(obf, n, L, S, **kw):
        return lambda name, expect: _uniform(name, "eligibility", obf, n, L, S, expect=expect, seed=len(name), **kw)

    el("el_obf_L8", "wave", u(True, 33, 8, 16))
    el("el_obf_L16", "tile", u(True, 33, 16, 24))
    PAIRS.append(("el_obf_L8", "el_obf_L16", "kernel"))
    el("el_deobf_L16", "wave", u(False, 33, 16, 8))
    el("el_deobf_L24", "tile", u(False, 33, 24, 16))
    PAIRS.append(("el_deobf_L16", "el_deobf_L24", "kernel"))
    el("el_L4096", "tile", u(True, 17, 4096, 4112))
    el("el_L4104", "wave", u(True, 17, 4104, 4112))
    PAIRS.append(("el_L4096", "el_L4104", "kernel"))
    el("el_instride4096", "tile", u(True, 17, 4088, 4096, in_stride=4096))
    el("el_instride4104", "wave", u(True, 17, 4088, 4096, in_stride=4104))
    PAIRS.append(("el_instride4096", "el_instride4104", "kernel"))
    el("el_base16", "tile", u(True, 17, 1200, 1216))
    el("el_base8", "wave", u(True, 17, 1200, 1216, in_align=8))
    PAIRS.append(("el_base16", "el_base8", "kernel"))
    el("el_slot_2p20", "tile", u(True, 3, 96, 1 << 20))
    el("el_slot_2p20_8", "wave", u(True, 3, 96, (1 << 20) + 8))
    PAIRS.append(("el_slot_2p20", "el_slot_2p20_8", "kernel"))
    el("el_W_eq_S", "tile", u(True, 17, 1200, 1208))
    el("el_W_gt_S", "wave", u(True, 17, 1200, 1200))            # every datagram dropped by the slot
    PAIRS.append(("el_W_eq_S", "el_W_gt_S", "drops"))
    el("el_pktcap_0", "tile", u(True, 17, 1200, 1216, pkt_cap=0))
    el("el_pktcap_W", "tile", u(True, 17, 1200, 1216, pkt_cap=1208))
    el("el_pktcap_W_8", "wave", u(True, 17, 1200, 1216, pkt_cap=1200))   # every datagram dropped by pkt_cap
    PAIRS.append(("el_pktcap_W", "el_pktcap_W_8", "drops"))
    PAIRS.append(("el_pktcap_0", "el_pktcap_W_8", "drops"))
    el("el_outcap_fit", "tile", u(True, 17, 1200, 1216, out_cap=16 * 1216 + 1208))
    el("el_outcap_short", "wave", u(True, 17, 1200, 1216, out_cap=16 * 1216 + 1207))   # the last one dropped
    PAIRS.append(("el_outcap_fit", "el_outcap_short", "drops"))
    top = M // 8 * 8
    el("el_outstride_max", "wave", u(True, 2, 96, top))
    el("el_outstride_over", INVALID, u(True, 2, 96, top + 8))
    PAIRS.append(("el_outstride_max", "el_outstride_over", "status"))
    for n in (1, 15, 16, 17):
        el("el_n%d_obf" % n, "tile", u(True, n, 1200, 1216))
    el("el_n17_deobf", "tile", u(False, 17, 1216, 1216))

    # ---- input_aliasing
    def al(name, fn):
        _reg("input_aliasing", name, lambda: fn(name))

    for L in (16, 1200, 1201):
        S = _r8(L + 8) + 8
        al("alias_bcast_L%d_slotted" % L, lambda name, L=L, S=S: _uniform(name, "input_aliasing", True, 33, L, S,
                                                                           in_stride=0, seed=L))
        al("alias_bcast_L%d_packed" % L, lambda name, L=L: _uniform(name, "input_aliasing", True, 33, L, 0,
                                                                     in_stride=0, seed=L))
    al("alias_bcast_deobf_L1200_slotted", lambda name: _uniform(name, "input_aliasing", False, 33, 1200, 1200, in_stride=0))
    al("alias_stride8_slotted", lambda name: _uniform(name, "input_aliasing", True, 33, 1200, 1216, in_stride=8))
    al("alias_stride8_packed", lambda name: _uniform(name, "input_aliasing", True, 33, 1200, 0, in_stride=8))
    al("alias_stride8_deobf_slotted", lambda name: _uniform(name, "input_aliasing", False, 33, 1200, 1200, in_stride=8))

    def offs(name, kind, S):
        n, L = 33, 1200
        off = np.full(n, 40, np.uint64) if kind == "equal" else (np.arange(n - 1, -1, -1, dtype=np.uint64) * 8)
        size = int(off.max()) + L
        cs = dict(name=name, family="input_aliasing", obf=True, n=n, inp=_bytes(9, size), in_off=off, in_len=None,
                  in_stride=0, len_uniform=L, out_cap=(n * S if S else n * (L + 8)) + 16, out_stride=S)
        return _finish(cs, ("auto", "wave"))

    for kind in ("equal", "descending"):
        al("alias_off_%s_slotted" % kind, lambda name, kind=kind: offs(name, kind, 1216))
        al("alias_off_%s_packed" % kind, lambda name, kind=kind: offs(name, kind, 0))


_register()


def build(name):
    cs = REGISTRY[name][1]()
    assert cs["name"] == name and cs["family"] == REGISTRY[name][0]
    return cs


def written_mask_stats(cs):
    """(written bytes, unwritten bytes) of the expected `out`."""
    w = sum(len(b) for _, b in cs["regions"])
    return w, cs["out_cap"] - w


def expected_out(cs):
    """The whole expected `out`: the caller's fill with the regions laid over it."""
    out = np.full(cs["out_cap"], SENTINEL, np.uint8)
    for off, b in cs["regions"]:
        out[off:off + len(b)] = np.frombuffer(b, np.uint8)
    return out


# ------------------------------------------------------------------ the case file of tests/emu/batch_main.cpp
# Settings the CPU tier leaves to the GPU tier: the flat kernel on the two contiguous
# batches that hold a 16 MiB datagram is over 1100 one-shot workgroups of 256 emulated
# threads each, about 80 s per case; AUTO and WAVE of the same cases take a second.
GPU_ONLY = {(name, "flat") for name in ("ladder_contig_a_obf", "ladder_contig_a_deobf", "ladder_contig_b_obf",
                                        "ladder_contig_b_deobf")}


def cpu_settings(cs):
    return [(s, k) for s, k in cs["settings"] if (cs["name"], s) not in GPU_ONLY]


def section(cs):
    """One batch section (tag 1), little-endian; the layout is in tests/emu/batch_main.cpp."""
    n = cs["n"]
    settings = cpu_settings(cs)
    name = cs["name"].encode()
    flags = (1 if cs["in_off"] is not None else 0) | (2 if cs["in_len"] is not None else 0)
    parts = [struct.pack("<II", 1, len(name)), name, struct.pack("<II", int(cs["obf"]), len(cs["psk"])), cs["psk"],
             struct.pack("<QIIQIIQQQ", n, flags, cs["in_align"], cs["in_stride"], cs["len_uniform"], cs["pkt_cap"],
                         cs["out_cap"], cs["out_stride"], len(cs["inp"])), cs["inp"].tobytes()]
    if cs["in_off"] is not None:
        parts.append(cs["in_off"].astype("<u8").tobytes())
    if cs["in_len"] is not None:
        parts.append(cs["in_len"].astype("<u4").tobytes())
    parts.append(cs["salts"].astype("<u8").tobytes())
    parts.append(struct.pack("<I", len(settings)))
    for s, k in settings:
        parts.append(struct.pack("<Ii", SETTING_ID[s], k if k == INVALID else KERNEL_ID[k]))
    parts.append(struct.pack("<i", cs["status"]))
    parts += [cs["out_off"].astype("<u8").tobytes(), cs["out_len"].astype("<u4").tobytes(),
              struct.pack("<QQ", cs["out_total"], len(cs["regions"]))]
    for off, b in cs["regions"]:
        parts += [struct.pack("<QQ", off, len(b)), b]
    return b"".join(parts)


def expected_lines(cs):
    return ["%s %s kernel=%d status=%d bad=0 first=-1 meta=0" % (
        cs["name"], s, k if k == INVALID else KERNEL_ID[k], cs["status"]) for s, k in cpu_settings(cs)]


def packet_vectors(L, seed=77):
    """The per-packet calls on L input bytes: (salt, payload of L bytes, its expected wire
    or b"" over the limit, a wire datagram of L bytes, its expected plain text or b"")."""
    salt = int(ref.splitmix64_at(seed, L)).to_bytes(8, "little")
    payload = ref.stream_bytes(seed, 0, L)
    wire = ref.obfuscate(PSK, payload, salt) if L <= M else b""
    wire_in = ref.obfuscate(PSK, payload[:L - 8], salt)
    plain = payload[:L - 8] if L <= M else b""
    assert len(wire_in) == L and (not plain or ref.deobfuscate(PSK, wire_in) == plain)
    return salt, payload, wire, wire_in, plain


def packet_section(L):
    """One per-packet section (tag 2) of the case file."""
    salt, payload, wire, wire_in, plain = packet_vectors(L)
    return b"".join([struct.pack("<II", 2, len(PSK)), PSK, struct.pack("<Q", L), salt, payload,
                     struct.pack("<Q", len(wire)), wire, wire_in, struct.pack("<Q", len(plain))])


def packet_line(L):
    return "packet L=%d obf=%d bad=0 deobf=%d bad=0" % (L, L + 8 if L <= M else 0, L - 8 if L <= M else 0)
