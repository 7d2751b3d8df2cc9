"""CPU tier of the ACL's hashed index over a DOMAIN_SET's FULL and ROOT values
(include/hyobfs_acl.h, "THE INDEX"; hysteria_amd/csrc/acl.hip, entry kind
kDomainIndex): the kernel itself through a stand-alone AddressSanitizer build
(tests/emu/acl_index_main.cpp + acl.hip against hip_emu.h, a child process; nothing
is preloaded), once as it is and once with a two-bit hash in which every probe
sequence is long and goes round the table's end; every group also compiled without
the index, with equal records; a seeded property run against tests/acl_ref.py; the
option struct's refusals; the Python surface's opt-in."""
import ctypes
import fcntl
import os
import subprocess

import pytest

import acl_cases as ac
import acl_index_cases as ic
import acl_ref
import acl_regex_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/llvm/bin/clang++"
BOTH = ic.FLAG_REGEX | ic.FLAG_INDEX


@pytest.fixture(scope="module")
def groups():
    return ic.groups()


# ------------------------------------------------------------------ the two emulated drivers
def _build(name, defines):
    if not os.path.exists(CLANG):
        pytest.skip("no host clang for the emulated build")
    csrc = os.path.join(ROOT, "hysteria_amd", "csrc")
    srcs = [os.path.join(EMU, "acl_index_main.cpp"), os.path.join(csrc, "acl.hip")]
    deps = srcs + [os.path.join(EMU, "hip_emu.h"), os.path.join(csrc, "kernels.h"), os.path.join(csrc, "acl_regex.h"),
                   os.path.join(ROOT, "include", "hyobfs_acl.h"), os.path.join(ROOT, "include", "hyobfs_sniff.h")]
    os.makedirs(os.path.join(EMU, "build"), exist_ok=True)
    exe = os.path.join(EMU, "build", name)
    with open(os.path.join(EMU, "build", "." + name + ".lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
            tmp = exe + ".tmp"
            subprocess.run([CLANG, "-std=c++20", "-O1", "-g", "-DHYOBFS_EMULATE", *defines, "-I" + EMU, "-I" + csrc, "-x",
                            "c++", "-fsanitize=address", "-fno-omit-frame-pointer", "-pthread",
                            "-Wno-unused-command-line-argument", *srcs, "-o", tmp], check=True, capture_output=True)
            os.replace(tmp, exe)
    return exe


@pytest.fixture(scope="module")
def main():
    """tests/emu/build/acl_index_main: acl.hip + the driver for the host under AddressSanitizer."""
    return _build("acl_index_main", [])


@pytest.fixture(scope="module")
def weak_main():
    """The same with -DHY_ACL_INDEX_HASH_BITS=2: four hash values in all."""
    return _build("acl_index_main_weak", ["-DHY_ACL_INDEX_HASH_BITS=2"])


def _run(exe, tmp_path, data, flags, index_min, *more):
    path = tmp_path / "cases.bin"
    path.write_bytes(data)
    r = subprocess.run([exe, str(path), str(flags), str(index_min), *[str(m) for m in more]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "done"
    return lines[:-1]


def _parse(groups, lines):
    """Per group: (entries of the walk table, {rule: (values, slots, max_probe)}, records)."""
    out, at = [], 0
    for g in groups:
        head = lines[at].split()
        assert head[:5] == ["group", "0", "-1", "-1", str(len(g[1]))], (g[0], lines[at])
        at += 1
        index = {}
        while at < len(lines) and lines[at].startswith("index "):
            r, values, slots, probe = (int(x) for x in lines[at].split()[1:])
            index[r] = (values, slots, probe)
            at += 1
        recs = [tuple(int(x) for x in ln.split()) for ln in lines[at:at + len(g[2])]]
        assert len(recs) == len(g[2])
        at += len(g[2])
        out.append((int(head[5]), index, recs))
    assert at == len(lines)
    return out


def _linear_entries(rules):
    return sum(len(r["entries"]) if r["kind"] == "domain_set" else 1 for r in rules)


def _check(exe, tmp_path, groups, mode, index_min, linear=True):
    """The groups through one entry point with the index: the restatement's records
    and the shape of the tables; with `linear`, also compiled without the index:
    the same records."""
    data = ac.case_file(groups, mode)
    with_index = _parse(groups, _run(exe, tmp_path, data, BOTH, index_min))
    without = _parse(groups, _run(exe, tmp_path, data, ic.FLAG_REGEX, 0)) if linear else None
    for k, g in enumerate(groups):
        exp = rc.expected(g, bool(mode), k)
        for i, (a, b) in enumerate(zip(with_index[k][2], exp)):
            assert a == b, (g[0], i, g[2][i], a, b)
        if linear:
            assert with_index[k][2] == without[k][2], g[0]
            assert without[k][:2] == (_linear_entries(g[1]), {}), g[0]
        for r, (values, slots, probe) in with_index[k][1].items():
            assert slots >= 2 * values and slots & (slots - 1) == 0 and 1 <= probe <= values, (g[0], r)
        if g[0] in ic.SHAPE:
            entries, index = ic.SHAPE[g[0]]
            assert with_index[k][0] == entries, g[0]
            assert {r: v[:2] for r, v in with_index[k][1].items()} == index, g[0]
    return with_index


# ------------------------------------------------------------------ the groups by the restatement alone
def test_case_groups_cover_their_edges(groups):
    exp = {g[0]: rc.expected(g) for g in groups}
    assert {g[0] for g in groups} >= {"ix_items_1", "ix_items_3", "ix_items_4", "ix_items_5", "ix_items_1029",
                                      "ix_boundary", "ix_empty", "ix_labels", "ix_threshold_3", "ix_threshold_65",
                                      "ix_mixed", "ix_straddle_62", "ix_straddle_63", "ix_straddle_64", "ix_straddle_65",
                                      "ix_never", "ix_big", "ix_cn"}
    #           value x.value xvalue value.x .value a..b a.b .b b ab ..b
    assert [e[1] for e in exp["ix_boundary"]][:11] == [2, 3, -1, -1, 3, 0, 1, 0, 1, -1, 0]
    #           onlyfull x.onlyfull both x.both twice y.twice ytwice x.y.value value. VALUE "" .
    assert [e[1] for e in exp["ix_boundary"]][11:] == [4, -1, 5, 5, 5, 5, -1, 3, 2, 2, -1, -1]
    assert [e[1] for e in exp["ix_empty"]] == [0, 1, 0, 1, -1, -1, -1, -1, -1, -1, 0, 1]
    assert [e[1] for e in exp["ix_labels"]][:5] == [0, 0, -1, -1, -1]
    assert {e[1] for e in exp["ix_labels"]} == {-1, 0, 1, 2, 3}
    for m in (3, 65):
        assert [e[1] for e in exp["ix_threshold_%d" % m]] == [0, 2, 0, 0, 1, 1, 2, 0, 1, 0, 2, -1]
    assert [e[1] for e in exp["ix_mixed"]] == [1, 1, 1, 0, 1, 1, -1, 2, -1] + [4, 3, 3, 3, 4, 4] + [4] * 6
    for n in (62, 63, 64, 65):
        assert [e[1] for e in exp["ix_straddle_%d" % n]] == [0, n - 1, -1, n, n, n + 1, n, n + 1, -1]
    assert [e[:2] for e in exp["ix_never"]] == [(0, -1)] * 8 + [(acl_ref.HOST, -1)] * 4 + [(0, 1)] * 3 + [(0, -1), (acl_ref.HOST, -1)]
    big = [e[1] for e in exp["ix_big"]]
    assert len(big) == 408 and big[:208:2] == [0] * 104 and big[1:200:2] == [0] * 100 and big[201:208:2] == [1] * 4
    assert big[208:] == [1] * 200
    assert len(exp["ix_items_1029"]) == 1029 and {e[1] for e in exp["ix_items_1029"]} == {-1, 0, 1}


# ------------------------------------------------------------------ the kernel under AddressSanitizer
@pytest.mark.parametrize("mode", (0, 1))
def test_emulated_kernel(main, tmp_path, groups, mode):
    """Every group through hyobfs_acl_match_batch (mode 0) and
    hyobfs_acl_match_sniffed_batch (mode 1) under AddressSanitizer, the bytes
    between names poisoned and `res` exactly n records long: the restatement's
    records, the walk table's entries and each rule's table as the cases pin them.
    Through match_batch every group is also compiled without the index and gives the
    same records (the sniffed form shares the walk; the GPU tier compares both)."""
    for m in sorted({ic.index_min(g[0]) for g in groups}):
        bucket = [g for g in groups if ic.index_min(g[0]) == m]
        got = _check(main, tmp_path, bucket, mode, m, linear=mode == 0)
        for g, (_, index, _) in zip(bucket, got):
            if g[0] == "ix_big":
                assert index[0][2] >= 2      # chains were walked
            if g[0] == "ix_threshold_65":
                assert sorted(index) == [1]   # 64 values under the default: not indexed; 65: indexed


def test_weak_hash(main, weak_main, tmp_path, groups):
    """Four hash values in all: every probe sequence begins in slots 0 to 3 and
    goes downwards, so all but the first four values lie round the table's end.
    The same records; the longest sequence is as long as its share of the values."""
    picked = [g for g in groups if g[0] in ("ix_boundary", "ix_mixed")] + ic.weak_groups()
    for mode in (0, 1):
        got = _check(weak_main, tmp_path, picked, mode, 1, linear=mode == 0)
        strong = _check(main, tmp_path, picked, mode, 1, linear=False)
        assert [g[2] for g in got] == [g[2] for g in strong]
    values, slots, probe = got[-1][1][0]
    assert (values, slots) == (40, 128) and probe >= 10
    assert strong[-1][1][0][2] < probe


def test_property_run(main, weak_main, tmp_path):
    """300 seeded sets of 1 to 12 FULL / ROOT values and 2,000 seeded names, both over
    {a, b, .} up to 8 bytes, against the restatement, with both binaries."""
    group = ic.property_group()
    assert len(group[1]) == 300 and len(group[2]) == 2000
    for exe in (main, weak_main):
        got = _check(exe, tmp_path, [group], 0, 1, linear=False)
        assert len(got[0][1]) == 300 and got[0][0] == 300
        assert 100 < sum(r[1] >= 0 for r in got[0][2]) < 1900


def test_opts_null_and_no_flag(main, tmp_path, groups):
    """opts == NULL is hyobfs_acl_ruleset_new; options without FLAG_INDEX compile as before."""
    picked = [g for g in groups if g[0] in ("ix_boundary", "ix_straddle_64")]
    data = ac.case_file(picked, 0)
    a, b = _run(main, tmp_path, data, "null", 0), _run(main, tmp_path, data, 0, 0)
    assert a == b and not any(ln.startswith("index") for ln in a)
    assert [ln.split()[5] for ln in a if ln.startswith("group")] == [str(_linear_entries(g[1])) for g in picked]


def test_emulated_creation_refusals(main, tmp_path):
    """The driver's view of the refusals: the option struct first, then rule and entry as before."""
    long_value = [("root", b"fine.test"), ("plain", b"p"), ("root", b"v" * 256), ("full", b"w" * 256)]
    groups = [("refused", [ac.R("exact", 1, pattern=b"fine.test"), ac.R("domain_set", 2, entries=long_value)], [])]
    data = ac.case_file(groups, 0)
    assert _run(main, tmp_path, data, BOTH, 1) == ["group -64 1 2 0 0"]
    assert _run(main, tmp_path, data, BOTH, 4) == ["group -64 1 2 0 0"]   # below the threshold: the linear entry refuses
    assert _run(main, tmp_path, data, 4, 0) == ["group -2 -1 -1 0 0"]
    assert _run(main, tmp_path, data, 8 | BOTH, 0) == ["group -2 -1 -1 0 0"]
    assert _run(main, tmp_path, data, ic.FLAG_REGEX, 1) == ["group -2 -1 -1 0 0"]   # index_min without the flag
    assert _run(main, tmp_path, data, BOTH, 1, 12, 0) == ["group -2 -1 -1 0 0"]     # struct_size
    assert _run(main, tmp_path, data, BOTH, 1, 20, 0) == ["group -2 -1 -1 0 0"]
    assert _run(main, tmp_path, data, BOTH, 1, 16, 1) == ["group -2 -1 -1 0 0"]     # reserved
    regex = [("root", b"a.test"), ("regex", b"^ok$")]
    data = ac.case_file([("regex", [ac.R("domain_set", 2, entries=regex)], [])], 0)
    assert _run(main, tmp_path, data, ic.FLAG_INDEX, 1) == ["group -63 0 1 0 0"]    # the REGEX bit is still needed


# ------------------------------------------------------------------ the library, no device needed
def test_option_struct_refusals():
    """hyobfs_acl_ruleset_new_opts checks the options, then the rules, all before the
    device is looked at; hyobfs_acl_ruleset_new_flags still refuses the INDEX bit."""
    from hysteria_amd import _lib, acl
    lib = acl._alib()
    arr, keep = ac.c_rules([ac.R("all", 1), ac.R("domain_set", 2, entries=[("root", b"a.test"), ("full", b"x" * 256)])])
    h = ctypes.c_void_p()

    def opts(struct_size=16, flags=acl.FLAG_INDEX, index_min=1, reserved=0):
        o = acl.HyobfsAclOptions(struct_size, flags, index_min, reserved)
        st = lib.hyobfs_acl_ruleset_new_opts(arr, 2, 0, ctypes.byref(o), ctypes.byref(h))
        return st, lib.hyobfs_acl_ruleset_bad_rule(), lib.hyobfs_acl_ruleset_bad_entry()
    assert ctypes.sizeof(acl.HyobfsAclOptions) == 16 and ctypes.sizeof(acl.HyobfsAclIndexInfo) == 16
    for bad in (dict(struct_size=12), dict(struct_size=0), dict(struct_size=32), dict(flags=4), dict(flags=acl.FLAG_INDEX | 8),
                dict(flags=0), dict(flags=acl.FLAG_REGEX), dict(reserved=1)):
        assert opts(**bad) == (_lib.HYOBFS_ERR_INVALID, -1, -1), bad
    for good in (dict(), dict(index_min=0), dict(index_min=2), dict(flags=0, index_min=0), dict(flags=3)):
        assert opts(**good) == (acl.ERR_PATTERN, 1, 1), good     # the options pass; the rule is refused, by name
    assert lib.hyobfs_acl_ruleset_new_flags(arr, 2, 0, 2, ctypes.byref(h)) == _lib.HYOBFS_ERR_INVALID
    assert lib.hyobfs_acl_ruleset_new_flags(arr, 2, 0, 3, ctypes.byref(h)) == _lib.HYOBFS_ERR_INVALID
    with pytest.raises(acl.RuleRefused) as e:
        acl.ruleset_new(arr, 2, 0, acl.FLAG_INDEX, index_min=1)
    assert (e.value.status, e.value.rule, e.value.entry) == (acl.ERR_PATTERN, 1, 1)
    # opts == NULL is hyobfs_acl_ruleset_new: the same status with or without a device
    arr, keep = ac.c_rules([ac.R("all", 1)])
    h2 = ctypes.c_void_p()
    a = lib.hyobfs_acl_ruleset_new_opts(arr, 1, 0, None, ctypes.byref(h))
    b = lib.hyobfs_acl_ruleset_new(arr, 1, 0, ctypes.byref(h2))
    assert a == b and a in (_lib.HYOBFS_OK, _lib.HYOBFS_ERR_NO_DEVICE)
    if a == _lib.HYOBFS_OK:
        assert lib.hyobfs_acl_ruleset_entries(h) == lib.hyobfs_acl_ruleset_entries(h2) == 1
        acl.ruleset_free(h)
        acl.ruleset_free(h2)
    assert lib.hyobfs_acl_ruleset_entries(None) == 0
    info = acl.HyobfsAclIndexInfo()
    assert lib.hyobfs_acl_ruleset_index_info(None, 0, ctypes.byref(info)) == _lib.HYOBFS_ERR_INVALID


def test_python_opt_in():
    """RuleSet and compile_rules hand the index over only on request; flags() says so."""
    from hysteria_amd import acl

    class Geo:
        def geoip(self, code):
            return None

        def geosite(self, name):
            return [("root", "a.test", []), ("full", "b.test", []), ("regex", "^c[0-9]\\.test$", [])]

    text = acl.parse_text_rules("x(geosite:any)\ny(all)")
    outs = {"x": 1, "y": 2}
    plain = acl.compile_rules(text, outs, Geo(), device_regex=True)
    assert (plain.device_index, plain.index_min, plain.flags()) == (False, 0, acl.FLAG_REGEX)
    rs = acl.compile_rules(text, outs, Geo(), device_regex=True, device_index=True, index_min=2)
    assert (rs.device_index, rs.index_min, rs.flags()) == (True, 2, acl.FLAG_REGEX | acl.FLAG_INDEX)
    assert acl.compile_rules(text[1:], outs, Geo(), device_index=True).flags() == acl.FLAG_INDEX
    assert [rs.match_host(n) for n in ("x.a.test", "x.b.test", "c7.test")] == [0, 1, 0]   # the host matcher is untouched
    with pytest.raises(ValueError):
        acl.RuleSet([], index_min=3)
    assert (acl.FLAG_INDEX, acl.INDEX_MIN_DEFAULT) == (2, 65)


def test_structs_and_constants(tmp_path):
    """The new constants, structs and entry points against the header, by a probe compiled with gcc."""
    from hysteria_amd import _lib, acl
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hyobfs_acl.h"\n'
                   '#ifdef SIGS\n'
                   'int (*f)(const hyobfs_acl_rule*, uint32_t, int, const hyobfs_acl_options*, hyobfs_acl_ruleset**) = '
                   'hyobfs_acl_ruleset_new_opts;\n'
                   'uint32_t (*g)(const hyobfs_acl_ruleset*) = hyobfs_acl_ruleset_entries;\n'
                   'int (*h)(const hyobfs_acl_ruleset*, uint32_t, hyobfs_acl_index_info*) = hyobfs_acl_ruleset_index_info;\n'
                   '#else\nint main(void){\n'
                   'printf("%u %u %d %zu %zu", HYOBFS_ACL_FLAG_INDEX, HYOBFS_ACL_INDEX_MIN_DEFAULT, HYOBFS_ABI_VERSION,\n'
                   '       sizeof(hyobfs_acl_options), sizeof(hyobfs_acl_index_info));\n'
                   'printf(" %zu %zu %zu %zu", offsetof(hyobfs_acl_options, struct_size), offsetof(hyobfs_acl_options, flags),\n'
                   '       offsetof(hyobfs_acl_options, index_min), offsetof(hyobfs_acl_options, reserved));\n'
                   'printf(" %zu %zu %zu %zu\\n", offsetof(hyobfs_acl_index_info, values), offsetof(hyobfs_acl_index_info, slots),\n'
                   '       offsetof(hyobfs_acl_index_info, max_probe), offsetof(hyobfs_acl_index_info, reserved));\n'
                   'return 0;}\n#endif\n')
    exe = tmp_path / "probe"
    gcc = ["gcc", "-std=c11", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)]
    subprocess.run(gcc + ["-DSIGS", "-c", "-o", str(tmp_path / "sigs.o")], check=True)   # the declared signatures
    subprocess.run(gcc + ["-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    o, i = acl.HyobfsAclOptions, acl.HyobfsAclIndexInfo
    assert out == [acl.FLAG_INDEX, acl.INDEX_MIN_DEFAULT, _lib.ABI_VERSION, ctypes.sizeof(o), ctypes.sizeof(i),
                   o.struct_size.offset, o.flags.offset, o.index_min.offset, o.reserved.offset,
                   i.values.offset, i.slots.offset, i.max_probe.offset, i.reserved.offset]
    for name in ("hyobfs_acl_ruleset_new_opts", "hyobfs_acl_ruleset_entries", "hyobfs_acl_ruleset_index_info"):
        assert name in _lib._ACL_SIG and name in _lib.header_functions()
