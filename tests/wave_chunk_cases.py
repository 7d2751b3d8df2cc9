"""The chunk-ownership lattice of the wave kernel (hysteria_amd/csrc/salamander_wave.h),
shared by the CPU tier (tests/test_wave_chunks.py through tests/emu/batch_main.cpp) and
the GPU tier (tests/test_gpu_wave_chunks.py).  The contiguous packed cases also reach the
opt-in flat kernel's general merge (salamander_flat.h).

Every case is built from the oracles alone and has the shape tests/batch_limit_cases.py
documents; the expected results, the case file's sections and the expected lines are
that module's (_finish, section, expected_out, expected_lines).  Every family asserts its
own coverage from the oracle's out_off / out_len when it is built: a builder that misses
a cell fails, not the kernel.

classify() restates in Python how the wave kernel sorts the 16-byte chunks of a wave's
group: inside one payload (swept), a boundary chunk of its first toucher that is complete
and that the sweep's lookup maps back to that lane (parked, while the group's slots last),
or stored late with a byte mask (incomplete, lookup elsewhere, out of slots).  It is used
only to assert that each class and each slot-count bucket occurs; expected bytes always
come from the oracle.

How many chunks a datagram and a run can park.  A parked chunk is complete and its first
toucher is the parking lane, so a parked first chunk starts on a chunk edge (st % 16 == 0).
Then the second chunk is a candidate only if the datagram ends inside it (W < 32), and the
third candidate (the last chunk, when it is neither) does not exist; with W >= 32 the
second chunk lies inside the payload and is swept.  Without the first chunk only two
candidates are left.  So a datagram parks at most two chunks (obfuscate: the chunk its
salt spills into and its last one, or its first and its last), never three, and on
deobfuscate at most one (there is no salt: the second chunk is a boundary only when it
is also the last).  A run's last datagram parks one fewer: no later lane of the wave
fills the chunk its end lies in (the next run is another wave's, or the output ends), and
when it ends on a chunk edge that chunk lies inside its payload and is swept.  A run of R
datagrams therefore parks at most 2 R - 1 chunks on obfuscate and R - 1 on deobfuscate
(classify() asserts both bounds for every case), and the reachable slot counts are:

  obfuscate    slotted and packed runs of 8 (64 datagrams per wave): up to 8 x 15 = 120;
               buckets 63, 64, 65 and a dense wave (80 slotted, 120 packed) all occur
               packed runs of 64 (the default, 32 datagrams per wave): at most 63 < kSlots,
               reached; the fallback cannot run
  deobfuscate  runs of 8: at most 8 x 7 = 56, reached slotted and packed; packed runs of 64:
               at most 31, reached; slotted runs of 64 (HYOBFS_RUN_LOG2 = 6): at most 63.
               `base + np` never reaches kSlots = 64 on deobfuscate, whatever the knobs

Families (NAMES[family] lists the case names, build(name) makes one):

  phase_width  every (output offset mod 32, width) pair at a group's first, last and an
               inner lane; widths 1..56 on deobfuscate, 8..56 on obfuscate (a wire datagram
               has its 8 salt bytes); free-form input with every input phase mod 16, and a
               contiguous copy
  neighbours   every ordered triple of 13 widths as consecutive datagrams, each at two
               or more chunk phases, triples across the 31|32, 127|128 and 255|256 edges
  crowded      runs of 2, 3, 15, 16, 17 and 40 datagrams of the smallest width (1 on
               deobfuscate, 8 on obfuscate) at phases 0, 1 and 15 and across the edges
  empty        runs of 1..300 dropped datagrams: an empty live group, an empty prefix
               tile, empty first and last groups, a chunk shared across an empty group
  slots        groups with 63, 64, 65 and the dense maximum of parkable chunks
  out_cap      one 96-datagram batch per out_cap within 17 bytes of the end of datagram
               31, 32 and 63
  strides      slotted output with strides that are no chunk multiples, full and ragged
"""
import functools

import numpy as np

import batch_limit_cases as bl
from batch_limit_cases import PSK, SENTINEL, expected_lines, expected_out, section  # noqa: F401  (the tiers use them)
from oracle import salamander_ref as ref

GROUP = 64            # lanes of a wave
DPW = 32              # datagrams per wave, packed runs of 64
SLOTS = 64            # kSlots, both layouts
TILE = 256            # datagrams per prefix tile
EDGES = (32, 128, 256)           # group, workgroup and prefix-tile edges (packed runs of 64)
MAX_N = 10000
MAX_OUT = 1 << 20


# ------------------------------------------------------------------ the restatement
def wave_lanes(n, packed, rl):
    """Per wave, the datagram of each live lane (a prefix of the 64 lanes)."""
    if packed and rl == 6:
        return [list(range(w * DPW, min(n, (w + 1) * DPW))) for w in range(-(-n // DPW))]
    ngroups = -(-n // GROUP)
    wt = -(-ngroups // 4) * 4
    waves = []
    for w in range(wt):
        lanes = []
        for lane in range(GROUP):
            r = (lane >> rl) * wt + w
            p = (r << rl) + (lane & ((1 << rl) - 1))
            if p < n:
                lanes.append(p)
        assert lanes == sorted(lanes)
        if lanes:
            waves.append(lanes)
    return waves


def _park_index(x, w, c):
    if w == 0:
        return 3
    cs, ce = x >> 4, (x + w - 1) >> 4
    return 0 if c == cs else 1 if (c == cs + 1 and cs + 1 <= ce) else 2 if (c == ce and ce > cs + 1) else 3


def classify(cs, rl=None, only=None):
    """The wave kernel's chunk classes, per wave, from the oracle's out_off / out_len.
    Offsets are real ones: a run's virtual offsets differ from them by a multiple of 128.
    Returns a list of dicts: lanes, parkable (chunks that ask for a slot), per lane `np`,
    swept / parked / late_partial / late_lookup / late_slots (chunk counts), chunks (the
    real chunks the wave touches), foreign_salt (an out-of-slots chunk holds salt bytes
    of a datagram other than its storing lane's).  only: that wave alone."""
    obf, n = cs["obf"], cs["n"]
    packed = cs["out_stride"] == 0
    if rl is None:
        rl = 6 if packed else 3
    run = 1 << rl
    salt = 8 if obf else 0
    off = [int(v) for v in cs["out_off"]]
    wid = [int(v) for v in cs["out_len"]]
    one_run = packed and rl == 6
    res = []
    for v, lanes in enumerate(wave_lanes(n, packed, rl)):
        if only is not None and v != only:
            continue
        m = len(lanes)
        # the runs of the wave: their 16-aligned base and the end of their written bytes
        x, run_of = [], []
        for i0 in range(0, m, DPW if one_run else run):
            ps = lanes[i0:i0 + (DPW if one_run else run)]
            rfirst = off[ps[0]] if packed else ps[0] * cs["out_stride"]
            rb = rfirst & ~15
            rend = max([off[p] + wid[p] for p in ps if wid[p]] + [rb])
            nch = (rend - rb + 15) >> 4
            x += [rb + min(off[p] - rb, nch << 4) for p in ps]
            run_of += [i0] * len(ps)
        w = [wid[p] for p in lanes]
        assert x == sorted(x)
        big = 1 << 62
        xs = x + [big] * (GROUP - m)
        ws = w + [0] * (GROUP - m)
        st = dict(lanes=lanes, parkable=0, np=[0] * m, swept=0, parked=0, late_partial=0, late_lookup=0,
                  late_slots=0, chunks=set(), foreign_salt=False, bytes=0)
        incm, pe_of = 0, []
        for k in range(m):
            pe_of.append(incm)
            incm = max(incm, x[k] + w[k] if w[k] else 0)
        pending = []          # (lane, chunk, complete and looked up here, holds a foreign salt)
        for k in range(m):
            if not w[k]:
                continue
            s, e = x[k], x[k] + w[k]
            c0, c1 = s >> 4, (e - 1) >> 4
            st["chunks"].update(range(c0, c1 + 1))
            cand = (c0, c0 + 1, c1)
            use = (pe_of[k] <= (c0 << 4), c0 + 1 <= c1, c1 > c0 + 1)
            for c in range(c0, c1 + 1):
                if s + salt <= (c << 4) and (c << 4) + 16 <= e:
                    st["swept"] += 1
                    st["bytes"] += 16
            for t in range(3):
                a = cand[t] << 4
                if not use[t] or (s + salt <= a and a + 16 <= e):
                    continue
                cov, foreign, j = 0, False, k
                while j < m and xs[j] < a + 16:
                    if ws[j]:
                        lo, hi = max(xs[j], a), min(xs[j] + ws[j], a + 16)
                        if lo < hi:
                            cov |= ((1 << (hi - lo)) - 1) << (lo - a)
                            if obf and j != k and max(xs[j], a) < min(xs[j] + 8, a + 16):
                                foreign = True
                    j += 1
                st["bytes"] += bin(cov).count("1")
                qq = 0                                   # group_search
                step = GROUP // 2
                while step:
                    qq = qq + step if xs[qq + step] <= a else qq
                    step >>= 1
                if ws[qq] and xs[qq] + ws[qq] > a:       # park_owner
                    o, ox, ow = qq, xs[qq], ws[qq]
                else:
                    o = qq + 1
                    ox, ow = (xs[o], ws[o]) if o < GROUP else (big, 0)
                back = o == k and _park_index(ox, ow, cand[t]) == t
                if cov != 0xFFFF:
                    st["late_partial"] += 1
                elif not back:
                    st["late_lookup"] += 1
                else:
                    st["np"][k] += 1
                    pending.append((k, foreign))
        base = 0
        for k in range(m):
            n_k = st["np"][k]
            over = base + n_k > SLOTS
            for kk, foreign in pending:
                if kk == k:
                    st["late_slots" if over else "parked"] += 1
                    st["foreign_salt"] |= over and foreign
            base += n_k
        st["parkable"] = base
        # every written byte of the wave is in exactly one swept or boundary chunk
        assert st["bytes"] == sum(w), (cs["name"], lanes[0], st["bytes"], sum(w))
        assert all(v <= (2 if obf else 1) for v in st["np"]), cs["name"]
        for i0 in set(run_of):                   # a run of R datagrams parks at most 2 R - 1 / R - 1 chunks
            R = run_of.count(i0)
            assert sum(v for v, r0 in zip(st["np"], run_of) if r0 == i0) <= (2 if obf else 1) * R - 1, cs["name"]
        res.append(st)
    return res


def class_totals(stats):
    return {k: sum(s[k] for s in stats) for k in ("swept", "parked", "late_partial", "late_lookup", "late_slots")}


# ------------------------------------------------------------------ building blocks
DROP = 0              # a width of 0 asks for a dropped datagram


def _lengths(obf, widths, pkt_cap):
    """Input lengths for the output widths; a dropped datagram gets a length the drop
    rules refuse (deobfuscate: 0..8 bytes, obfuscate: L + 8 > pkt_cap)."""
    lens = []
    for i, W in enumerate(widths):
        if W == DROP:
            lens.append(pkt_cap - 7 + i % 3 if obf else (i * 5) % 9)
        else:
            assert W >= (8 if obf else 1)
            lens.append(W - 8 if obf else W + 8)
    return lens


def _input(obf, lens, seed, contig, salts, step=1):
    """The input bytes and offsets: back to back (contiguous), or free-form with gaps of
    0..6 bytes in front of each datagram (`step` picks them), none behind the last."""
    parts, off, pos = [], np.zeros(len(lens), np.uint64), 0
    for i, L in enumerate(lens):
        if not contig:
            gap = (i * step + seed) % 7
            parts.append(np.full(gap, 0x3C, np.uint8))
            pos += gap
        off[i] = pos
        parts.append(bl._bytes(seed * 100003 + i, L) if obf else bl._wire(PSK, seed * 100003 + i, L, salts[i]))
        pos += L
    inp = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return inp, off


def _case(name, family, obf, widths, *, contig=False, stride=0, seed=1, out_cap=None, settings=None, step=1):
    """A batch of the given output widths (DROP: a dropped datagram): packed (stride 0) or
    slotted, free-form or contiguous input.  out_cap defaults to the last written byte."""
    n = len(widths)
    assert n <= MAX_N
    uncut = out_cap is None
    drops = any(W == DROP for W in widths)
    pkt_cap = max(64, max(widths)) if (obf and drops) else 0
    lens = _lengths(obf, widths, pkt_cap)
    salts = ref.splitmix64_array(2, seed, n)
    inp, off = _input(obf, lens, seed, contig, salts, step)
    if out_cap is None:
        if stride:
            last = max(i for i, W in enumerate(widths) if W)
            out_cap = max(last * stride + widths[last], (n - 1) * stride + 1)
        else:
            out_cap = sum(widths)
    assert out_cap <= MAX_OUT
    if settings is None:
        settings = ("auto", "wave", "flat") if (contig and not stride) else ("auto", "wave")
    cs = dict(name=name, family=family, obf=obf, n=n, inp=inp, in_off=None if contig else off,
              in_len=np.array(lens, np.uint32), in_stride=0, len_uniform=0, salts=salts, out_cap=out_cap,
              out_stride=stride, pkt_cap=pkt_cap)
    cs = bl._finish(cs, settings)
    want = dict(cs["settings"])
    assert want["auto"] == "wave" and want["wave"] == "wave" and want.get("flat", "flat") == "flat", name
    if uncut:
        assert [int(v) for v in cs["out_len"]] == list(widths), name     # the oracle agrees with the plan
    return cs


def _d(obf):
    return "obf" if obf else "deobf"


def _wmin(obf):
    return 8 if obf else 1


def _fill(obf, cur, phase, lo=16):
    """A filler width of lo..lo+15 that moves the output offset `cur` to `phase` mod 16."""
    return lo + (phase - cur - lo) % 16


# ------------------------------------------------------------------ 1. phase x width
PW_WMAX = 56
PW_CASE_N = 9984                  # 312 groups of 32


def _lane_class(i):
    return 0 if i % DPW == 0 else 2 if i % DPW == DPW - 1 else 1


@functools.lru_cache(maxsize=None)
def phase_width_plan(obf):
    """Greedy width lists, one per case: the next width hits an uncovered (phase mod 32,
    width, lane class) cell where the current phase has one, else moves to a phase that
    has one for the next lane.  All cells are hit (asserted again from the oracle)."""
    widths = list(range(_wmin(obf), PW_WMAX + 1))
    left = [[set(widths) for _ in range(32)] for _ in range(3)]
    remaining = 3 * 32 * len(widths)
    plans = []
    while remaining:
        plan, pos = [], 0
        while len(plan) < PW_CASE_N and (remaining or len(plan) % DPW):
            i = len(plan)
            c, ph, cn = _lane_class(i), pos % 32, _lane_class(i + 1)
            open_here = left[c][ph]
            pool = open_here if open_here else widths
            best = None
            for W in pool:
                if left[cn][(ph + W) % 32]:
                    best = W
                    break
            if best is None:
                best = next(iter(pool)) if open_here else widths[(i * 7) % len(widths)]
            if best in open_here:
                open_here.discard(best)
                remaining -= 1
            plan.append(best)
            pos += best
        # the tail: a payload of 16 bytes or more that ends one byte into a chunk, so the last
        # chunk's window has to be clamped; the free-form input ends at that payload's last byte
        plan.append(24 + (1 - pos - 24) % 16)
        plans.append(plan)
    return plans


def phase_width_cells(cs):
    """The (phase mod 32, width, lane class) cells of a case, from the oracle."""
    return {(int(o) % 32, int(w), _lane_class(i)) for i, (o, w) in enumerate(zip(cs["out_off"], cs["out_len"])) if w}


def _phase_width(name, obf, k, contig):
    cs = _case(name, "phase_width", obf, phase_width_plan(obf)[k], contig=contig, seed=11 + k, step=3)
    end = int(cs["out_off"][-1]) + int(cs["out_len"][-1])
    assert int(cs["out_len"][-1]) - (8 if obf else 0) >= 16 and end % 16 == 1 and end == cs["out_cap"], name
    if not contig:
        assert {int(o) % 16 for o in cs["in_off"]} == set(range(16)), name
    start = int(cs["in_len"][:-1].astype(np.uint64).sum()) if contig else int(cs["in_off"][-1])
    assert start + int(cs["in_len"][-1]) == len(cs["inp"]), name      # the input ends at the last payload's last byte
    return cs


# ------------------------------------------------------------------ 2. neighbours
NB_WIDTHS = {False: (DROP, 1, 2, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33),
             # obfuscate writes 8 salt bytes: 1, 2 and 7 cannot occur; payloads of 2, 17 and 33 bytes stand in
             True: (DROP, 8, 9, 10, 15, 16, 17, 24, 25, 31, 32, 33, 41)}


def de_bruijn(k, n):
    """The lexicographically least de Bruijn sequence B(k, n) (Lyndon words)."""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return seq


def neighbour_triples(cs):
    """{(w0, w1, w2): the chunk phases at which that triple of widths starts}."""
    w = [int(v) for v in cs["out_len"]]
    o = [int(v) for v in cs["out_off"]]
    seen = {}
    for i in range(len(w) - 2):
        seen.setdefault((w[i], w[i + 1], w[i + 2]), set()).add(o[i] % 16)
    return seen


def _neighbours(name, obf):
    alpha = NB_WIDTHS[obf]
    seq = de_bruijn(len(alpha), 3)
    one = [alpha[s] for s in seq + seq[:2]]
    widths = one + [_wmin(obf) + 4] + one + [_wmin(obf) + 9] + one       # three passes, the phase moved between them
    cs = _case(name, "neighbours", obf, widths, seed=5)
    seen = neighbour_triples(cs)
    for t in ((a, b, c) for a in alpha for b in alpha for c in alpha):
        assert len(seen.get(t, ())) >= 2, (name, t, seen.get(t))
    w = [int(v) for v in cs["out_len"]]
    for e in EDGES:                       # triples of the alphabet across every edge, both ways
        assert all(set(w[i:i + 3]) <= set(alpha) for i in (e - 2, e - 1)), (name, e)
    return cs


# ------------------------------------------------------------------ 3. crowded chunks
CROWD_K = (2, 3, 15, 16, 17, 40)
CROWD_PHASES = (0, 1, 15)


def crowded_runs(cs):
    """[(first index, length, phase mod 16)] of the maximal runs of the smallest width."""
    wc = _wmin(cs["obf"])
    w = [int(v) for v in cs["out_len"]]
    runs, i = [], 0
    while i < len(w):
        if w[i] == wc:
            j = i
            while j < len(w) and w[j] == wc:
                j += 1
            runs.append((i, j - i, int(cs["out_off"][i]) % 16))
            i = j
        else:
            i += 1
    return runs


def _crowded(name, obf, contig):
    wc = _wmin(obf)
    widths, pos = [], 0

    def add(W):
        nonlocal pos
        widths.append(W)
        pos += W

    def run(k, phase, at=None):
        """k smallest datagrams from output phase `phase`; at: the index of the run's first."""
        while at is not None and len(widths) % TILE != (at - 1) % TILE:
            add(16 + (len(widths) * 5) % 31)
        add(_fill(obf, pos, phase, 17))
        for _ in range(k):
            add(wc)

    for k in CROWD_K:
        for phase in CROWD_PHASES:
            run(k, phase)
    for e in EDGES:                      # runs across the group, workgroup and tile edges
        run(3, 15, at=e - 1)
        run(40 if e > 32 else 17, 1, at=e + TILE - 9)
    add(33)
    cs = _case(name, "crowded", obf, widths, contig=contig, seed=7)
    runs = crowded_runs(cs)
    assert {(k, ph) for _, k, ph in runs} >= {(k, ph) for k in CROWD_K for ph in CROWD_PHASES}, name
    for e in EDGES:
        assert any(i % e != 0 and i // e != (i + k - 1) // e for i, k, _ in runs), (name, e)
    most = 16 if not obf else 2
    per_chunk = np.bincount((cs["out_off"][cs["out_len"] > 0] // 16).astype(np.int64))
    assert per_chunk.max() >= most, name       # 16 datagrams (deobfuscate) / two salts (obfuscate) start in one chunk
    return cs


# ------------------------------------------------------------------ 4. empty stretches
EMPTY_RUNS = (1, 31, 32, 33, 64, 65, 256, 300)


def dropped_runs(cs):
    """[(first index, length)] of the maximal runs of dropped datagrams."""
    w = [int(v) for v in cs["out_len"]]
    runs, i = [], 0
    while i < len(w):
        if w[i] == 0:
            j = i
            while j < len(w) and w[j] == 0:
                j += 1
            runs.append((i, j - i))
            i = j
        else:
            i += 1
    return runs


def _empty(name, obf, contig):
    small = _wmin(obf) + 5               # 13 / 6 bytes: neighbours share chunks
    widths = [DROP] * DPW                # the batch's first group is empty

    def valid(k):
        for _ in range(k):
            widths.append(small + (len(widths) * 3) % 23)

    def until(mod, rem):
        while len(widths) % mod != rem:
            valid(1)

    valid(3)
    for D in EMPTY_RUNS:
        if D in (32, 64):
            until(DPW, 0)                # whole groups, live and empty
        elif D == 33:
            until(DPW, DPW - 1)
        elif D == 256:
            until(TILE, 0)               # a whole prefix tile of width 0
        if D not in (32, 64, 256):
            widths.append(small)         # ends inside a chunk
        widths += [DROP] * D
        valid(2)
    until(DPW, DPW - 1)                  # a chunk shared across an empty group
    widths.append(small + 1)
    widths += [DROP] * DPW
    valid(5)
    until(DPW, 0)
    widths += [DROP] * DPW               # the batch's last group is empty
    cs = _case(name, "empty", obf, widths, contig=contig, seed=9)
    w = np.array([int(v) for v in cs["out_len"]])
    n = len(w)
    runs = dropped_runs(cs)
    assert {k for _, k in runs} >= set(EMPTY_RUNS), (name, sorted({k for _, k in runs}))
    empty_groups = [g for g in range(n // DPW) if not w[g * DPW:(g + 1) * DPW].any()]
    assert 0 in empty_groups and n // DPW - 1 in empty_groups and n % DPW == 0, name
    assert any(0 < g < n // DPW - 1 for g in empty_groups), name
    assert any(not w[t * TILE:(t + 1) * TILE].any() for t in range(1, n // TILE)), name
    shared = False                       # valid, a whole empty group, valid: the two share a chunk
    for i, k in runs:
        g0 = -(-i // DPW)
        if i > 0 and i + k < n and (g0 + 1) * DPW <= i + k and int(cs["out_off"][i + k]) % 16:
            shared = True
    assert shared, name
    lens = cs["in_len"][w == 0]
    assert (lens == 0).any() or obf
    assert (lens > 0).any(), name        # dropped lengths that advance a contiguous input
    return cs


# ------------------------------------------------------------------ 5. slot pressure
SLOT_BUCKETS = (63, 64, 65)


def _layout(widths, stride):
    off, pos = [], 0
    for i, W in enumerate(widths):
        off.append(i * stride if stride else pos)
        pos += W
    return off


def _count(obf, widths, stride, rl, v):
    cs = dict(name="tuning", obf=obf, n=len(widths), out_stride=stride, out_off=_layout(widths, stride), out_len=widths)
    return classify(cs, rl, only=v)[0]["parkable"]


def _tune(obf, widths, stride, rl, targets):
    """Moves wave v's parkable count to targets[v] (None: left as it is), a step at a time.
    Slotted: a datagram loses its last byte (its last chunk gets a gap).  Packed: the edge
    between two datagrams of a run moves by 1..24 bytes (the offsets after them stay).
    Either way only the wave of that datagram changes: a wave's classes depend on its own
    lanes alone."""
    widths = list(widths)
    waves = wave_lanes(len(widths), stride == 0, rl)
    for v, target in enumerate(targets):
        if target is None:
            continue
        count = _count(obf, widths, stride, rl, v)
        for _ in range(4):
            for p in waves[v]:
                if count == target:
                    break
                for step in ((-1,) if stride else (-1, 1, -2, 2, -7, 7, -8, 8, -16, 16, -24, 24)):
                    trial = list(widths)
                    if stride:
                        trial[p] -= 1
                    elif p % (1 << rl) == 0:
                        break
                    else:
                        trial[p - 1] += step
                        trial[p] -= step
                    if trial[p] < _wmin(obf) or (not stride and trial[p - 1] < _wmin(obf)):
                        continue
                    got = _count(obf, trial, stride, rl, v)
                    if abs(got - target) < abs(count - target):
                        widths, count = trial, got
                        break
        assert count == target, (v, count, target)
    return widths


SLOT_MAX = {(True, "packed"): 2 * DPW - 1, (False, "packed"): DPW - 1,       # the bounds of the module docstring
            (True, "slotted"): 120, (True, "packed8"): 120, (False, "slotted"): 56, (False, "packed8"): 56}
SLOT_RL = {"slotted": 3, "packed8": 3, "packed": 6}


def slot_counts(cs, layout):
    """The parkable chunks per wave of a slots case under the run length it is built for."""
    return [s["parkable"] for s in classify(cs, SLOT_RL[layout])]


def _slots(name, obf, layout):
    n = 4 * GROUP
    rl = SLOT_RL[layout]
    if layout == "slotted":                      # runs of 8 (HYOBFS_RUN_LOG2 = 3, the default)
        stride = 25 if obf else 18               # deobfuscate: 8 x 18 bytes are 9 chunks, 7 of them hold an edge
        widths = _tune(obf, [stride] * n, stride, rl, list(SLOT_BUCKETS) + [None]) if obf else [stride] * n
    elif layout == "packed8":                    # packed, runs of 8 (HYOBFS_PACKED_RUN_LOG2 = 3, CPU tier)
        stride = 0
        widths = _tune(obf, [9] + [32] * (n - 1), 0, rl, list(SLOT_BUCKETS) + [None]) if obf else [18] * n
    else:                                        # packed, runs of 64: 32 datagrams per wave
        stride = 0
        widths = ([25] + [32] * (DPW - 1)) * (n // DPW) if obf else [7] + [32] * (n - 1)
    cs = _case(name, "slots", obf, widths, stride=stride, seed=13)
    counts = slot_counts(cs, layout)
    if obf and layout != "packed":
        assert counts[:3] == list(SLOT_BUCKETS) and 65 < counts[3] <= SLOT_MAX[obf, layout], (name, counts)
        stats = classify(cs, rl)
        assert any(s["late_slots"] for s in stats) and any(s["foreign_salt"] for s in stats), name
    else:                                        # the layout's maximum, below kSlots, is reached
        assert max(counts) == SLOT_MAX[obf, layout] < SLOTS, (name, counts)
    return cs


# ------------------------------------------------------------------ 6. out_cap cuts
CUT_AFTER = (31, 32, 63)
CUT_SPAN = 17


def _cut_widths(obf):
    return [_wmin(obf) + (i * 37 + 11) % 49 for i in range(96)]


def _out_cap_case(name, obf, after, delta):
    widths = _cut_widths(obf)
    E = sum(widths[:after + 1])
    cs = _case(name, "out_cap", obf, widths, seed=17, out_cap=E + delta)
    w = [int(v) for v in cs["out_len"]]
    end = np.cumsum(widths)
    assert all((w[i] == widths[i]) == (end[i] <= E + delta) and w[i] in (0, widths[i]) for i in range(96)), name
    assert [int(v) for v in cs["out_off"]] == [0] + [int(v) for v in end[:-1]], name    # a cut moves no offset
    return cs


# ------------------------------------------------------------------ 7. slotted strides
STRIDES = (9, 15, 16, 17, 24, 31, 33, 47, 80, 1201)
STRIDE_N = 64 * 4 * 3 + 5


def _stride_case(name, obf, stride, ragged):
    lo = _wmin(obf)
    if ragged:
        widths = [DROP if (i % 41 == 17 and stride > 9) else lo + (i * 29 + 3) % (stride - lo + 1) for i in range(STRIDE_N)]
        widths[-1] = max(lo, stride - 3)
        for i in range(7, STRIDE_N, 16):         # every other run's last slot is full: it reaches the next wave's run
            widths[i] = stride
    else:
        widths = [stride] * STRIDE_N
    cs = _case(name, "strides", obf, widths, stride=stride, seed=19)
    stats = classify(cs)
    shared = set()
    for a in range(len(stats)):
        for b in range(a + 1, len(stats)):
            shared |= stats[a]["chunks"] & stats[b]["chunks"]
    if stride % 2:                               # a run of 8 slots starts inside a chunk
        assert shared, name                      # chunks that two waves write parts of
    if ragged:
        assert bl.written_mask_stats(cs)[1] > 0 and (np.array(cs["out_len"]) < stride).any(), name
    return cs


# ------------------------------------------------------------------ the registry
REGISTRY = {}
NAMES = {f: [] for f in ("phase_width", "neighbours", "crowded", "empty", "slots", "out_cap", "strides")}


def _reg(family, name, fn):
    assert name not in REGISTRY
    REGISTRY[name] = (family, fn)
    NAMES[family].append(name)


def _register():
    for obf in (True, False):
        d = _d(obf)
        for k in range(len(phase_width_plan(obf))):
            for contig in (False, True):
                nm = "pw_%s_%d_%s" % (d, k, "contig" if contig else "free")
                _reg("phase_width", nm, lambda nm=nm, obf=obf, k=k, contig=contig: _phase_width(nm, obf, k, contig))
        _reg("neighbours", "nb_" + d, lambda d=d, obf=obf: _neighbours("nb_" + d, obf))
        for contig in (False, True):
            c = "contig" if contig else "free"
            _reg("crowded", "crowd_%s_%s" % (d, c), lambda d=d, obf=obf, contig=contig, c=c: _crowded(
                "crowd_%s_%s" % (d, c), obf, contig))
            _reg("empty", "empty_%s_%s" % (d, c), lambda d=d, obf=obf, contig=contig, c=c: _empty(
                "empty_%s_%s" % (d, c), obf, contig))
        for layout in ("slotted", "packed", "packed8"):
            nm = "slots_%s_%s" % (d, layout)
            _reg("slots", nm, lambda nm=nm, obf=obf, layout=layout: _slots(nm, obf, layout))
        for after in CUT_AFTER:
            for delta in range(-CUT_SPAN, CUT_SPAN + 1):
                nm = "cut_%s_e%d_%+d" % (d, after, delta)
                _reg("out_cap", nm, lambda nm=nm, obf=obf, after=after, delta=delta: _out_cap_case(nm, obf, after, delta))
        for stride in STRIDES:
            for ragged in (False, True):
                nm = "stride_%s_%d_%s" % (d, stride, "ragged" if ragged else "full")
                _reg("strides", nm, lambda nm=nm, obf=obf, stride=stride, ragged=ragged: _stride_case(nm, obf, stride, ragged))


_register()


@functools.lru_cache(maxsize=None)
def build(name):
    cs = REGISTRY[name][1]()
    assert cs["name"] == name and cs["family"] == REGISTRY[name][0]
    assert cs["n"] <= MAX_N and cs["out_cap"] <= MAX_OUT
    return cs


def contiguous_packed(name):
    return name.endswith("_contig")


def cpu_settings(name):
    """The settings of a case the CPU tier runs; the GPU tier runs them all.  An emulated
    workgroup is 256 threads that meet at a barrier for every shuffle, about 0.15 s for
    128 datagrams, and the 24 phase_width cases are 1790 workgroups a setting.  So on the
    CPU each free-form phase_width case runs under WAVE, and its contiguous copy under AUTO,
    which is the same kernel with the input offsets from the length scan, and under FLAT
    with hashers (a few seconds a case; without hashers, where every tile hashes its own
    keys, it is some 40 s, so that run takes the last, shorter pair).  The out_cap cuts are
    96 datagrams each, but every launch also runs the two scan kernels."""
    if REGISTRY[name][0] == "out_cap":           # 210 launches of three kernels each: WAVE, and AUTO where the cut is at E
        return ("auto", "wave") if name.endswith("+0") else ("wave",)
    if REGISTRY[name][0] != "phase_width":
        return ("auto", "wave", "flat")
    return ("auto", "flat") if contiguous_packed(name) else ("wave",)


def last_phase_width_pair(obf):
    """The names of the direction's last, shortest phase_width pair (free-form, contiguous)."""
    return ["pw_%s_%d_%s" % (_d(obf), len(phase_width_plan(obf)) - 1, c) for c in ("free", "contig")]
