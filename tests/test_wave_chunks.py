"""CPU tier of the wave kernel's chunk-ownership lattice (tests/wave_chunk_cases.py): the
builder's own coverage, and every case through tests/emu/batch_main.cpp, the stand-alone
AddressSanitizer program of tests/test_batch_limits.py, linked and run the same way (a
child process with its own main, nothing preloaded; every array in an allocation of
exactly the promised size).  Settings: AUTO and WAVE, FLAT (with 4 hasher workgroups and
with none) for the contiguous packed copies, less what wave_chunk_cases.cpu_settings
leaves to the GPU tier for the two largest families, and the wave kernel again under the
run-length knobs HYOBFS_RUN_LOG2 / HYOBFS_PACKED_RUN_LOG2, which are read once
per process and so stay a matter of this tier."""
import os
import subprocess

import numpy as np
import pytest

import batch_limit_cases as bl
import wave_chunk_cases as wc
from test_batch_limits import batch_main  # noqa: F401  (the fixture that builds the driver)

M = bl.M


# ------------------------------------------------------------------ the builder's own coverage
@pytest.mark.parametrize("obf", [True, False], ids=["obf", "deobf"])
@pytest.mark.parametrize("layout", ["free", "contig"])
def test_phase_width_cells(obf, layout):
    """Every (output offset mod 32, width, first / inner / last lane) cell occurs, counted
    from the oracle's out_off / out_len: 32 x 56 x 3 on deobfuscate, 32 x 49 x 3 on
    obfuscate (widths 8..56)."""
    cells = set()
    for name in wc.NAMES["phase_width"]:
        if name.startswith("pw_%s_" % wc._d(obf)) and name.endswith(layout):
            cells |= wc.phase_width_cells(wc.build(name))
    want = {(ph, W, c) for ph in range(32) for W in range(wc._wmin(obf), wc.PW_WMAX + 1) for c in range(3)}
    assert want <= cells, sorted(want - cells)[:8]
    assert len(want) == 32 * (49 if obf else 56) * 3


def test_families_meet_their_conditions():
    """Every other family builds (each builder asserts its own triples, runs, straddles,
    stretches, buckets and cuts) and stays small; every chunk class of the restatement
    occurs in every family it can occur in; the slot-count buckets 63, 64, 65 and a dense
    maximum occur where the layout reaches them."""
    assert sorted(wc.REGISTRY) == sorted(n for names in wc.NAMES.values() for n in names)
    for family, names in wc.NAMES.items():
        assert names, family
        if family in ("phase_width", "out_cap"):
            continue
        for d in ("_obf", "_deobf"):
            tot = dict.fromkeys(("swept", "parked", "late_partial", "late_lookup", "late_slots"), 0)
            for name in names:
                if d + "_" in name or name.endswith(d):
                    for k, v in wc.class_totals(wc.classify(wc.build(name))).items():
                        tot[k] += v
            assert tot["swept"] and tot["parked"] and tot["late_partial"], (family, d, tot)
            assert tot["late_lookup"] == 0      # the sweep's lookup finds every complete chunk's first toucher
    for name in ("cut_obf_e31_-17", "cut_deobf_e32_+0", "cut_obf_e63_+17", "cut_deobf_e63_-1"):
        cs = wc.build(name)
        assert (cs["out_len"] == 0).any() and cs["out_total"] <= cs["out_cap"]
    cuts = {d: [wc.build("cut_%s_e%d_%+d" % (d, a, k)) for a in wc.CUT_AFTER for k in range(-17, 18)]
            for d in ("obf", "deobf")}
    for d, cases in cuts.items():
        slack = {c["out_cap"] - c["out_total"] for c in cases}
        assert 0 in slack and max(slack) > 1        # cut exactly at a datagram's end, and inside the next one
        widths = wc._cut_widths(d == "obf")
        ends = set(np.cumsum(widths))
        assert any(c["out_cap"] + 1 in ends for c in cases), d       # one byte short of a datagram's end
    # slot pressure: obfuscate, slotted and packed runs of 8, reaches every bucket and overflows; packed runs of
    # 64 and every deobfuscate layout reach their maximum, which is below kSlots (wave_chunk_cases' docstring)
    for layout in ("slotted", "packed8"):
        cs = wc.build("slots_obf_" + layout)
        stats = wc.classify(cs, wc.SLOT_RL[layout])
        counts = wc.slot_counts(cs, layout)
        assert counts[:3] == [63, 64, 65] and counts[3] > 65, (layout, counts)
        assert [bool(s["late_slots"]) for s in stats] == [False, False, True, True], layout
        assert any(s["foreign_salt"] for s in stats), layout
        assert max(wc.slot_counts(wc.build("slots_deobf_" + layout), layout)) == 56
    assert max(wc.slot_counts(wc.build("slots_obf_packed"), "packed")) == 63
    assert max(wc.slot_counts(wc.build("slots_deobf_packed"), "packed")) == 31
    # deobfuscate never asks for the 64th slot, whatever the run length the knobs set
    for name in wc.NAMES["slots"] + wc.NAMES["strides"] + wc.NAMES["neighbours"] + wc.NAMES["crowded"]:
        if "_deobf" in name:
            cs = wc.build(name)
            for rl in ((0, 3, 6) if cs["out_stride"] else (0, 3, 5, 6)):
                assert all(s["parkable"] < wc.SLOTS for s in wc.classify(cs, rl)), (name, rl)
    # a datagram parks two chunks at most, on deobfuscate one: the fallback needs more than 32 datagrams per wave
    for name in wc.NAMES["neighbours"] + wc.NAMES["crowded"] + wc.NAMES["empty"]:
        assert all(s["parkable"] <= wc.SLOTS and not s["late_slots"] for s in wc.classify(wc.build(name))), name


def test_restatement_on_known_layouts():
    """classify() on layouts small enough to check by hand."""
    def stats(obf, widths, stride=0, rl=None):
        cs = dict(name="hand", obf=obf, n=len(widths), out_stride=stride, out_off=wc._layout(widths, stride), out_len=widths)
        return wc.classify(cs, rl)
    # one deobfuscated datagram of 48 bytes: three chunks inside its payload
    s, = stats(False, [48])
    assert (s["swept"], s["parked"], s["late_partial"]) == (3, 0, 0)
    # obfuscate, 48 bytes: the salt's chunk is a complete boundary chunk of its first toucher
    s, = stats(True, [48])
    assert (s["swept"], s["parked"], s["late_partial"]) == (2, 1, 0)
    # 40 + 24 bytes: chunk 2 holds the end of one payload and the next salt: parked by the first toucher
    s, = stats(True, [40, 24])
    assert (s["swept"], s["parked"], s["late_partial"], s["np"]) == (2, 2, 0, [2, 0])
    # a batch that ends inside a chunk: that chunk is late
    s, = stats(True, [40])
    assert (s["swept"], s["parked"], s["late_partial"]) == (1, 1, 1)
    # sixteen one-byte datagrams fill one chunk: the first owns it
    s, = stats(False, [1] * 16)
    assert (s["swept"], s["parked"], s["np"][0]) == (0, 1, 1)
    # slotted, stride 24: runs of 8 (192 bytes) of four waves; 5 datagrams are wave 0's first run
    s, = stats(True, [24] * 5, stride=24)
    assert s["lanes"] == [0, 1, 2, 3, 4] and s["parkable"] == 5 and s["late_partial"] == 1


# ------------------------------------------------------------------ the emulated kernels
def _run(exe, tmp_path, sections, env_extra, timeout=900):
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for s in sections:
            f.write(s)
    env = {k: v for k, v in os.environ.items() if not k.startswith("HYOBFS_")}     # the driver sets the kernel itself
    env["HYOBFS_FLAT_HASHERS"] = "4"
    env.update(env_extra)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=timeout, env=env)
    os.unlink(path)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert lines[0] == "limit=%d" % M and lines[-1] == "done"
    return lines[1:-1]


def _check(exe, tmp_path, names, only=None, env=None):
    """The named cases under their settings (only: that subset of them) in one child."""
    want, sections = [], []
    for name in names:
        cs = wc.build(name)
        keep = wc.cpu_settings(name) if only is None else only
        cs = dict(cs, settings=[(s, k) for s, k in cs["settings"] if s in keep])
        if not cs["settings"]:
            continue
        want += wc.expected_lines(cs)
        sections.append(wc.section(cs))
    assert sections
    got = _run(exe, tmp_path, sections, env or {})
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:6]


def _groups(names, size):
    return [names[i:i + size] for i in range(0, len(names), size)]


_SMALL = [f for f in wc.NAMES if f not in ("phase_width", "out_cap")]
# the knobs' other values; (6, 3) is the default the tests above run.  Packed runs of 64,
# 32, 8 and 1 datagrams; slotted runs of 64, 8 and 1.
KNOBS = [dict(HYOBFS_PACKED_RUN_LOG2="0", HYOBFS_RUN_LOG2="0"), dict(HYOBFS_PACKED_RUN_LOG2="3", HYOBFS_RUN_LOG2="6"),
         dict(HYOBFS_PACKED_RUN_LOG2="5", HYOBFS_RUN_LOG2="3")]
_KNOB_IDS = ["packed0_slotted0", "packed3_slotted6", "packed5_slotted3"]


@pytest.mark.parametrize("names", _groups(wc.NAMES["phase_width"], 2), ids=lambda g: g[0])
def test_emulated_phase_width(batch_main, tmp_path, names):  # noqa: F811
    """Output phase x width x lane class: the free-form case under WAVE, its contiguous copy
    under AUTO and FLAT (wave_chunk_cases.cpu_settings says why; the GPU tier runs every
    setting).  The input ends at the last payload's last byte and that payload's last chunk
    needs the clamped window (the builder asserts both), so an unclamped window read is an
    AddressSanitizer error."""
    _check(batch_main, tmp_path, names)


@pytest.mark.parametrize("family", _SMALL)
def test_emulated_family(batch_main, tmp_path, family):  # noqa: F811
    """Neighbours, crowded chunks, empty stretches, slot pressure and slotted strides under
    AUTO and WAVE, the contiguous packed copies under FLAT too."""
    _check(batch_main, tmp_path, wc.NAMES[family])


@pytest.mark.parametrize("after", wc.CUT_AFTER)
def test_emulated_out_cap_cuts(batch_main, tmp_path, after):  # noqa: F811
    """out_cap at every byte within 17 of the end of datagram 31, 32 and 63 under WAVE (AUTO
    too where the cut is at that end; the GPU tier runs both everywhere): out is exactly
    out_cap bytes (a store past it is an AddressSanitizer error), offsets never move."""
    _check(batch_main, tmp_path, [n for n in wc.NAMES["out_cap"] if "_e%d_" % after in n])


@pytest.mark.parametrize("names", [[n for n in wc.REGISTRY if wc.contiguous_packed(n) and n.startswith(p)]
                                   for p in (wc.last_phase_width_pair(True)[1], wc.last_phase_width_pair(False)[1], "crowd",
                                             "empty")], ids=lambda g: g[0])
def test_emulated_flat_without_hashers(batch_main, tmp_path, names):  # noqa: F811
    """The contiguous packed copies under FLAT with every tile hashing its own keys."""
    _check(batch_main, tmp_path, names, only=("flat",), env=dict(HYOBFS_FLAT_HASHERS="0"))


@pytest.mark.parametrize("knobs", KNOBS, ids=_KNOB_IDS)
@pytest.mark.parametrize("names", [["pw_obf_0_free", "pw_deobf_0_free", wc.last_phase_width_pair(True)[1], wc.last_phase_width_pair(False)[1]]]
                         + [wc.NAMES[f] for f in _SMALL], ids=lambda g: g[0])
def test_emulated_run_lengths(batch_main, tmp_path, names, knobs):  # noqa: F811
    """Families 2-5 and 7, and of the phase_width family the first free-form and the last
    contiguous case of each direction, through the wave kernel with other run lengths: the
    packed shorter-run branch has its own scan and its own salt index in the late stores."""
    _check(batch_main, tmp_path, names, only=("wave",), env=knobs)
