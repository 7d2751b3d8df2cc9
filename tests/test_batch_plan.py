"""CPU tier of the Salamander batch calls' launch plan: which kernel runs and how much
scratch a batch needs, over a lattice with the smallest values on both sides of every
predicate of the plan (tests/emu/plan_main.cpp walks it; nothing is launched).

tests/golden/batch_plan.json is the table recorded from the commit before the plan
became one function (`python tests/test_batch_plan.py` records it): the distinct rows
and, per environment, the table as runs (row id, count, row id, count, ...) in the
program's order.  The test builds the program against the current emulated library, runs
it once per environment as a child process with nothing preloaded, and compares row for
row."""
import fcntl
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_build  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
FIXTURE = os.path.join(ROOT, "tests", "golden", "batch_plan.json")
CLANG = "/opt/rocm/llvm/bin/clang++"
M = (1 << 24) - 64
INVALID = -2

# plan_main.cpp's lattice, outermost axis first
AXES = [("out", 2), ("out_stride", 6), ("salts", 2), ("n", 7), ("input", 5), ("workspace", 3), ("in", 2),
        ("out_cap", 2), ("pkt_cap", 2), ("len_uniform", 2)]
SHAPE = [s for _, s in AXES]
N = [0, 1, 2, 255, 256, 257, 65537]
STRIDE = [0, 1201, 1208, 4096, M, M + 1]
EXPLICIT, STRIDED_UNIFORM, STRIDED_LEN, CONTIGUOUS, BROADCAST = range(5)
# the knobs are read once per process: one child process per environment
ENVS = {"clean": {}, "wave": {"HYOBFS_KERNEL": "wave"}, "flat": {"HYOBFS_KERNEL": "flat"},
        "run3": {"HYOBFS_PACKED_RUN_LOG2": "3"}}


def _plan_main():
    """tests/emu/build/plan_main, rebuilt when the driver, the header or the emulated
    library is newer."""
    lib = emu_build.ensure_emu_lib()
    src = os.path.join(EMU, "plan_main.cpp")
    deps = [src, lib, os.path.join(ROOT, "include", "hyobfs.h")]
    os.makedirs(os.path.join(EMU, "build"), exist_ok=True)
    exe = os.path.join(EMU, "build", "plan_main")
    with open(os.path.join(EMU, "build", ".plan_main.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
            tmp = exe + ".tmp"
            subprocess.run([CLANG, "-std=c++20", "-O1", "-g", "-fsanitize=address", "-fno-omit-frame-pointer", "-pthread",
                            src, "-L" + EMU, "-lhyobfs_emu", "-Wl,-rpath," + EMU, "-o", tmp], check=True,
                           capture_output=True)
            os.replace(tmp, exe)
    return exe


def _table(exe, extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("HYOBFS_")}
    env.update(extra)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert lines[0] == "rows=%d" % np.prod(SHAPE) and lines[-1] == "done"
    return lines[1:-1]


def _encode(tables):
    rows, runs = {}, {}
    for name, lines in tables.items():
        r = runs[name] = []
        for line in lines:
            i = rows.setdefault(line, len(rows))
            if r and r[-2] == i:
                r[-1] += 1
            else:
                r += [i, 1]
    return {"rows": list(rows), "runs": runs}


def _decode(fix):
    return {name: [fix["rows"][i] for i, c in zip(r[::2], r[1::2]) for _ in range(c)] for name, r in fix["runs"].items()}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return _decode(json.load(f))


def test_plan_table_equals_the_recorded_one(recorded):
    if not os.path.exists(CLANG):
        pytest.skip("no host clang for the emulated build")
    exe = _plan_main()
    assert sorted(recorded) == sorted(ENVS)
    for name, extra in ENVS.items():
        got, want = _table(exe, extra), recorded[name]
        assert len(got) == len(want)
        assert got == want, (name, [(np.unravel_index(i, SHAPE), g, w)
                                    for i, (g, w) in enumerate(zip(got, want)) if g != w][:6])


def _arrays(recorded):
    """Per environment: the workspace bytes and the eight answers, shaped by the lattice."""
    out = {}
    for name, lines in recorded.items():
        a = np.array([[int(x) for x in line.split()] for line in lines], np.int64)
        assert a.shape == (np.prod(SHAPE), 9)
        out[name] = a.reshape(SHAPE + [9])
    return out


def test_recorded_table_is_not_flat(recorded):
    """Every kernel value and HYOBFS_ERR_INVALID occur; the five prepass shapes occur,
    told apart by the workspace size and the kernel; every value of every axis of the
    lattice differs from another value of that axis in at least one row, and so does every
    environment from the clean one."""
    tab = _arrays(recorded)
    assert {int(v) for a in tab.values() for v in np.unique(a[..., 1:])} == {0, 1, 2, 3, INVALID}
    for ax, (name, size) in enumerate(AXES):
        for i in range(size):       # (explicit offsets and a stride with in_len are one case to the plan)
            assert any((np.take(a, i, ax) != np.take(a, j, ax)).any() for a in tab.values() for j in range(size)), (name, i)
    for name in ("wave", "flat", "run3"):
        assert (tab[name] != tab["clean"]).any(), name

    idx = np.indices(SHAPE)
    n = np.array(N)[idx[3]]
    stride = np.array(STRIDE)[idx[1]]
    layout, in_mis, half = idx[4], idx[6], idx[7]
    out_cap = (n * np.where(stride == 0, 1209, stride)) >> half
    tsums = ((n + 255) // 256 + 1) * 8
    flat_ws = ((16 + 24 * ((out_cap + 16383) // 16384 + 1) + 255) & ~255) + 256 + 64 * n
    ok = (idx[0] == 0) & (idx[2] == 0) & (idx[5] == 1) & (n > 0)     # out aligned, salts, the promised workspace
    auto_obf = {name: a[..., 1] for name, a in tab.items()}          # context setting 0, obfuscate
    ws = {name: a[..., 0] for name, a in tab.items()}
    packed = stride == 0

    def seen(env, where, size, kernels):
        sel = ok & where
        assert sel.any()
        assert (ws[env][sel] == size[sel]).all(), env
        assert set(np.unique(auto_obf[env][sel])) == kernels, (env, np.unique(auto_obf[env][sel]))

    slotted = (stride > 0) & (stride <= M)
    # no prepass: slotted output, explicit or strided input -- the tile kernel or the wave kernel
    seen("clean", slotted & (layout != CONTIGUOUS), 0 * n, {1, 2})
    # width sums and their scan: packed output, explicit or strided input
    seen("clean", packed & (layout != CONTIGUOUS), tsums, {1})
    # contiguous input: one datagram is an ordinary strided batch
    cont = (layout == CONTIGUOUS) & (n > 1)
    # width and length sums scanned in the packed launch (the flat kernel, not eligible from
    # misaligned input, adds nothing to the promise there)
    seen("clean", packed & cont & (in_mis == 1), 2 * tsums, {1})
    # length sums, their scan and the input offsets: into slots, or shortened packed runs
    seen("clean", slotted & cont, 2 * tsums + 8 * n, {1})
    seen("run3", packed & cont & (in_mis == 1), 2 * tsums + 8 * n, {1})
    # the flat kernel's sums, scan and locate prepass; the promise covers it under every setting
    seen("flat", packed & cont & (in_mis == 0), 2 * tsums + flat_ws, {3})
    seen("clean", packed & cont & (in_mis == 0), 2 * tsums + flat_ws, {1})
    assert (tab["clean"][..., 7][ok & packed & cont & (in_mis == 0)] == 3).all()    # context setting FLAT (3), obfuscate


if __name__ == "__main__":      # records the fixture from the library built from the working tree
    exe = _plan_main()
    with open(FIXTURE, "w") as f:
        json.dump(_encode({name: _table(exe, extra) for name, extra in ENVS.items()}), f, separators=(",", ":"))
        f.write("\n")
    print(os.path.getsize(FIXTURE), "bytes")
