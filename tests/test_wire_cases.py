"""CPU tier of the realm punch matcher and the Gecko parse and encode kernels: the
edge lattices of tests/wire_cases.py through tests/emu/wire_main.cpp, a stand-alone
AddressSanitizer program linked against the emulated library (tests/emu/
libhyobfs_emu.so) and run as a child process.  Every array sits in an allocation of
exactly its size, so a byte read or written past the API's promise ends the run."""
import fcntl
import os
import subprocess
import sys

import pytest

import wire_cases as wc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_build  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def wire_main():
    """tests/emu/build/wire_main, rebuilt when the driver, a header or the emulated
    library is newer."""
    if not os.path.exists(CLANG):
        pytest.skip("no host clang for the emulated build")
    lib = emu_build.ensure_emu_lib()
    src = os.path.join(EMU, "wire_main.cpp")
    deps = [src, lib] + [os.path.join(ROOT, "include", h) for h in ("hyobfs.h", "hyobfs_gecko.h", "hyobfs_realm.h")]
    os.makedirs(os.path.join(EMU, "build"), exist_ok=True)
    exe = os.path.join(EMU, "build", "wire_main")
    with open(os.path.join(EMU, "build", ".wire_main.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
            tmp = exe + ".tmp"
            subprocess.run([CLANG, "-std=c++20", "-O1", "-g", "-fsanitize=address", "-fno-omit-frame-pointer", "-pthread",
                            src, "-L" + EMU, "-lhyobfs_emu", "-Wl,-rpath," + EMU, "-o", tmp], check=True,
                           capture_output=True)
            os.replace(tmp, exe)
    return exe


def _run(exe, tmp_path, data, timeout=300):
    path = tmp_path / "cases.bin"
    path.write_bytes(data)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "done"
    return lines[:-1]


# ------------------------------------------------------------------ the builders' own conditions
def test_lattices_meet_their_conditions():
    lat = wc.punch_lattice()
    n = len(lat["len"])
    assert sum(lbl.startswith("flip bit") for lbl in lat["labels"]) == 264
    assert sum(e[0] >= 0 for e in lat["exp"]) >= 70 and sum(e[0] < 0 for e in lat["exp"]) >= 270
    assert {e[0] for e in lat["exp"]} == {-1, 0, 1, 3, 4}        # attempt 2 duplicates attempt 1: never reported
    absent = lat["real"] == 0
    assert sorted(lat["len"][absent].tolist()) == sorted(wc.PUNCH_ABSENT_LENGTHS)
    assert (lat["off"][absent] == len(lat["buf"])).all()
    assert int((lat["off"] + lat["len"])[~absent].max()) == len(lat["buf"])    # no slack
    assert len({(int(o), int(ln)) for o, ln in zip(lat["off"][~absent], lat["len"][~absent])}) == n - absent.sum() - 2
    par = wc.parse_lattice()
    assert par["counts"] == {"empty": 5120, "pass": 22016, "truncated": 10338, "invalid": 11050, "fragment": 631}
    assert int((par["off"] + par["len"]).max()) == len(par["buf"])
    cases = wc.encode_cases()
    assert len(cases) == 36
    for cs in cases:
        fr = cs["frames"]
        assert int((fr["chunk_off"] + fr["chunk_len"]).max()) == len(cs["msg"])           # chunks end at msg's end
        assert cs["out_len"] >= int((cs["off"] + 13 + fr["pad_len"] + fr["chunk_len"]).max())
    wires = {int(w) for cs in cases if cs["mode"] == "limit"
             for w in 13 + cs["frames"]["pad_len"].astype(int) + cs["frames"]["chunk_len"].astype(int)}
    assert wires == {2046, 2047, 2048, 2049, 2050}


def test_case_dtypes_match_the_bindings():
    from hysteria_amd import gecko, realm
    assert wc.FRAME_DTYPE == gecko.FRAME_DTYPE and wc.PARSED_DTYPE == gecko.PARSED_DTYPE
    assert realm.ATTEMPT_DTYPE.itemsize == len(wc.attempts_bytes(wc.punch_lattice()["attempts"][:1]))
    assert wc.PARSE_STATUS == {"pass": gecko.PASS, "fragment": gecko.FRAGMENT, "empty": gecko.EMPTY,
                               "truncated": gecko.ERR_TRUNCATED, "invalid": gecko.ERR_INVALID}


# ------------------------------------------------------------------ realm
def test_emulated_punch_lattice(wire_main, tmp_path):
    """Every run of the lattice (whole, prefixes of 1 / 255 / 256 / 257 entries, no
    attempts with `attempts` null, `type` and `padding` null): match, type and padding
    of every entry, zero on a miss; gaps between the datagrams poisoned, entries of an
    out-of-range length pointing at the end of the buffer."""
    runs = wc.punch_runs()
    lines = _run(wire_main, tmp_path, b"".join(wc.punch_section(n, m, null) for _, n, m, null in runs))
    lat = wc.punch_lattice()
    at = 0
    for name, n, m, null in runs:
        assert lines[at] == "punch n=%d m=%d" % (n, m), name
        exp = wc.punch_expected(n, m)
        for i in range(n):
            j, t, pad = exp[i]
            want = (j, 0xEE, 0xEEEEEEEE) if null else (j, t, pad)     # null outputs: the driver's own fill
            assert tuple(int(x) for x in lines[at + 1 + i].split()) == want, (name, i, lat["labels"][i])
        at += 1 + n
    assert at == len(lines)


# ------------------------------------------------------------------ Gecko parse
def test_emulated_parse_lattice(wire_main, tmp_path):
    """All six fields of every record of the lattice; every byte after a datagram's
    last poisoned, the buffer ending with a two-byte datagram."""
    lat = wc.parse_lattice()
    assert _run(wire_main, tmp_path, wc.parse_section()) == ["parse n=%d bad=0 first=-1" % len(lat["len"])]


# ------------------------------------------------------------------ Gecko encode
@pytest.mark.parametrize("mode", wc.ENCODE_MODES)
def test_emulated_encode_layouts(wire_main, tmp_path, mode):
    """The whole `out` of every layout case of one mode, `msg` and `out` without slack."""
    cases = [cs for cs in wc.encode_cases() if cs["mode"] == mode]
    lines = _run(wire_main, tmp_path, b"".join(wc.encode_section(cs) for cs in cases))
    assert lines == ["encode n=%d out=%d bad=0 first=-1" % (cs["n"], cs["out_len"]) for cs in cases], \
        [cs["name"] for cs, ln in zip(cases, lines) if "bad=0" not in ln]


@pytest.mark.parametrize("name", ["straddle32_ascending", "straddle32_shuffled", "straddle38_ascending",
                                  "straddle38_shuffled", "span24_aligned", "span31_window", "span32_window"])
def test_emulated_encode_far_offsets(wire_main, tmp_path, name):
    """out_off around 2^32 and 2^38 and groups spanning 2^31 and 2^32, `out` a sparse
    mapping: the frames' bytes and 100 sentinel bytes on either side.  The aligned
    sweep crosses a gap of 2^24 bytes here (5500 steps of the 64 emulated lanes);
    span31_aligned, the same group with a gap of 2^31 - 2000 bytes, runs on the GPU only
    (tests/test_gpu_gecko.py): its 700k steps, each a few barrier rounds of 64 threads,
    take this tier from minutes to over half an hour depending on the machine."""
    cs = wc.far_cases()[name]
    nbytes = sum(len(e) for _, e in cs["windows"])
    assert _run(wire_main, tmp_path, wc.far_section(cs)) == [
        "far n=%d windows=%d bytes=%d bad=0 first=-1" % (len(cs["frames"]), len(cs["windows"]), nbytes)]
