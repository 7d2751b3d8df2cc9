"""CPU tier of the sniffer's HTTP branch and TCP dispatch (include/hyobfs_sniff.h,
rules H0-H7): the Python restatement (tests/http_ref.py) against the
reference's own requests, the kernel itself through a stand-alone
AddressSanitizer build (tests/emu/http_main.cpp + sniff.hip + quic.hip against
hip_emu.h, run as a child process), and the Python surface without a GPU."""
import collections
import fcntl
import json
import os
import struct
import subprocess

import pytest

import http_cases as hc
import http_ref
import sni_ref
import sniff_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(ROOT, "tests", "golden", "http_sniff_vectors.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------ the restatement
def test_restatement_reference_http_vectors(vectors):
    """sniff_test.go:47-52 and :74-77: example.com from a Host with and without a port."""
    from hysteria_amd.sniff import Sniffer
    for v in vectors["http"]:
        data = v["data"].encode("latin-1")
        st, name_len, name_off, need, name = http_ref.http_request_host(data)
        assert (st, name, need) == (0, v["host"].encode(), 0)
        assert data[name_off:name_off + name_len] == name
        assert http_ref.tcp_sniff(data) == (st, name_len, name_off, need, name)
        assert Sniffer._rewrite(v["req_addr"], name) == v["rewritten"]
    # the reference's other inputs (sniff_test.go:96, :105): letters first, so the HTTP
    # branch reads on for a request line; two bytes are too few to tell
    assert http_ref.tcp_sniff(b"Wait It's All Ohio? Always Has Been.")[0] == http_ref.NEED_MORE
    assert http_ref.tcp_sniff(b"\x01\x02\x03\x04\x05\x06\x07\x08\x09\x0a")[0] == http_ref.UNRECOGNIZED
    assert http_ref.tcp_sniff(b"\x01\x02") == (http_ref.NEED_MORE, 0, 0, 3, b"")


def test_restatement_statuses_of_the_lattice():
    """Spot checks that pin the restatement's reading of the rules."""
    exp = {n: http_ref.http_request_host(m) for n, m in hc.lattice_cases()}
    R = http_ref
    want = {
        "h0_len_2": R.NOT_HTTP, "h0_len_3": R.NEED_MORE, "h0_digit_third": R.NOT_HTTP, "h1_one_space": R.MALFORMED,
        "h2_method_paren": R.MALFORMED, "h2_method_tchars": 0, "h3_http_1_10": R.MALFORMED, "h3_http_11": R.MALFORMED,
        "h3_lower": R.MALFORMED, "h4_star": 0, "h4_empty_uri": R.MALFORMED, "h4_double_slash": 0,
        "h4_pct_at_end": R.MALFORMED, "h4_pct_zz_path": R.MALFORMED, "h4_pct_zz_query": 0, "h4_ctl": R.MALFORMED,
        "h4_del": R.MALFORMED, "h4_absolute": R.HOST, "h4_connect": R.HOST, "h4_absolute_bad_proto": R.MALFORMED,
        "h5_first_line_space": R.MALFORMED, "h5_folded": R.HOST, "h5_folded_then_bad": R.HOST,
        "h5_bad_then_folded": R.MALFORMED, "h5_no_colon": R.MALFORMED, "h5_key_paren": R.MALFORMED,
        "h5_empty_key_good": 0, "h5_empty_key_bad": R.MALFORMED, "h5_value_bare_cr": R.MALFORMED,
        "h5_value_nul": R.MALFORMED, "h5_value_0x80": 0, "h5_lf_only": 0, "h6_host_case": 0, "h6_two_hosts": R.MALFORMED,
        "h6_two_hosts_te": R.MALFORMED, "h6_te": R.HOST, "h6_trailer": R.HOST, "h6_two_cl": R.HOST, "h6_cl_1x": R.HOST,
        "h6_cl_18": 0, "h6_cl_19": R.HOST, "h6_cl_bad_need_more": R.NEED_MORE, "h7_empty_host": R.HOST,
        "h7_name_256": R.NAME_CAP,
    }
    for n, st in want.items():
        assert exp[n][0] == st, (n, exp[n])
    assert exp["h5_key_space"][:3] == (0, 0, 0)          # "Host : x" is not a Host header
    assert exp["h6_host_empty"][:3] == exp["h6_no_host"][:3] == (0, 0, 0)
    names = {"h7_port": b"a", "h7_v6_port": b"::1", "h7_v6_no_port": b"[::1]", "h7_colons": b"a:b:c",
             "h7_after_bracket": b"[a]b:1", "h7_stray_rb": b"a]:1", "h7_dot_end": b"example.com.", "h7_ip": b"10.0.0.1"}
    for n, name in names.items():
        assert exp[n][0] == 0 and exp[n][4] == name, (n, exp[n])
    big = {n: http_ref.http_request_host(m) for n, m in hc.big_window_cases()}
    assert big["win_big_final_lf_262143"][:2] == (0, 11)
    assert big["win_big_final_lf_262144"][0] == big["win_big_no_end_262144"][0] == R.MALFORMED
    assert big["win_big_no_end_262143"][:4] == (R.NEED_MORE, 0, 0, 262144)
    assert big["win_big_bad_line_past_limit"][0] == R.MALFORMED


def test_split_host_agrees_with_the_package():
    """http_ref.split_host and hysteria_amd.sniff.split_host_port restate the same function."""
    from hysteria_amd.sniff import split_host_port
    vals = [m.split(b"Host: ", 1)[1].split(b"\r\n")[0] for n, m in hc.lattice_cases() if n.startswith("h7_")]
    assert len(vals) > 20
    for v in vals:
        got = http_ref.split_host(v)
        try:
            want = split_host_port(v.decode("latin-1"))[0].encode("latin-1")
        except ValueError:
            want = None
        assert (got[1] if got else None) == want, v


def test_fuzz_set_is_balanced():
    """Of the 512 mutations at least 15 % stay OK with a name, at least 15 % are
    malformed, at least 5 % are left to the host and at least 5 % need more
    bytes, by the restatement alone."""
    cases = hc.fuzz_cases()
    assert len(cases) == 512
    kinds = collections.Counter((e[0], e[1] > 0) for e in hc.expected(cases, http_ref.http_request_host))
    assert kinds[(0, True)] >= 77 and kinds[(http_ref.MALFORMED, False)] >= 77, kinds
    assert kinds[(http_ref.HOST, False)] >= 26 and kinds[(http_ref.NEED_MORE, False)] >= 26, kinds


def test_window_cases_cover_the_edges():
    """The request line's LF, the Host line's start, its colon and its value at
    each byte around a 64-byte step's and a 1024-byte stage's edge."""
    exp = dict(zip((n for n, _ in hc.window_cases()), hc.expected(hc.window_cases(), http_ref.http_request_host)))
    for k in (62, 63, 64, 65, 127, 128):
        assert exp[f"win_reqline_lf_{k}"][:2] == (0, 11)
    starts = {int(n[12:]) for n in exp if n.startswith("win_host_at_") and n[12:].isdigit()}
    for edge in (64, 128, 1024):
        # the key (+0..3), the colon (+4) and the value (+6..21) each begin on both sides of the edge
        assert set(range(edge - 12, edge + 2)) <= starts, edge
    for n, e in exp.items():
        if n.startswith("win_host_at_"):
            assert e[0] == 0 and e[4] == b"example.com", n
    assert exp["win_final_lf_last"][0] == 0 and exp["win_one_short"][0] == http_ref.NEED_MORE
    assert exp["win_bare_cr_63"][0] == exp["win_bare_cr_63_in_key"][0] == http_ref.MALFORMED
    assert exp["win_line_ends_63_folded"][0] == http_ref.HOST


# ------------------------------------------------------------------ the kernel on the CPU
@pytest.fixture(scope="module")
def http_main():
    """tests/emu/build/http_main: sniff.hip + quic.hip + the driver, compiled for
    the host with AddressSanitizer (a program with its own main: nothing is
    preloaded).  Rebuilt when a source is newer."""
    if not os.path.exists(CLANG):
        pytest.skip("no host clang for the emulated build")
    csrc = os.path.join(ROOT, "hysteria_amd", "csrc")
    srcs = [os.path.join(EMU, "http_main.cpp"), os.path.join(csrc, "sniff.hip"), os.path.join(csrc, "quic.hip")]
    deps = srcs + [os.path.join(EMU, "hip_emu.h"), os.path.join(csrc, "kernels.h"), os.path.join(csrc, "sha256.h"),
                   os.path.join(csrc, "quic_crypto.h"), os.path.join(csrc, "sniff_http.h"),
                   os.path.join(ROOT, "include", "hyobfs_sniff.h"), os.path.join(ROOT, "include", "hyobfs_quic.h")]
    os.makedirs(os.path.join(EMU, "build"), exist_ok=True)
    exe = os.path.join(EMU, "build", "http_main")
    with open(os.path.join(EMU, "build", ".http_main.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
            tmp = exe + ".tmp"
            subprocess.run([CLANG, "-std=c++20", "-O1", "-g", "-DHYOBFS_EMULATE", "-I" + EMU, "-I" + csrc, "-x", "c++",
                            "-fsanitize=address", "-fno-omit-frame-pointer", "-pthread",
                            "-Wno-unused-command-line-argument", *srcs, "-o", tmp], check=True, capture_output=True)
            os.replace(tmp, exe)
    return exe


def _run(exe, tmp_path, mode, msgs, stride=hc.NAME_STRIDE):
    path = tmp_path / f"cases{mode}.bin"
    path.write_bytes(struct.pack("<3I", mode, len(msgs), stride) + b"".join(struct.pack("<I", len(m)) + m for m in msgs))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "tail a5 " + "ff" * 16      # the byte after names and the record after res[n - 1]
    assert len(lines) == len(msgs) + 1
    return lines[:-1]


def _check(names, exp, lines, stride=hc.NAME_STRIDE):
    """Status, name_len, name_off, need, the name row and its untouched tail."""
    assert len(lines) == len(exp)
    for name, e, line in zip(names, exp, lines):
        f = line.split()
        assert tuple(int(x) for x in f[:4]) == e[:4], (name, f[:4], e[:4])
        row = bytes.fromhex(f[4]) if stride else b""
        assert row == e[4] + bytes([hc.SENTINEL]) * (stride - len(e[4])), name


def _both(exe, tmp_path, cases, stride=hc.NAME_STRIDE):
    names, msgs = [n for n, _ in cases], [m for _, m in cases]
    _check(names, hc.expected(cases, http_ref.http_request_host, stride), _run(exe, tmp_path, 0, msgs, stride), stride)
    _check(names, hc.expected(cases, http_ref.tcp_sniff, stride), _run(exe, tmp_path, 1, msgs, stride), stride)


def test_emulated_lattice_cases(http_main, tmp_path):
    """The rule lattice through both entry points under AddressSanitizer, the
    gaps between streams poisoned."""
    _both(http_main, tmp_path, list(hc.lattice_cases()))


def test_emulated_window_cases(http_main, tmp_path):
    """The step, stage and end-of-input edges through both entry points."""
    _both(http_main, tmp_path, list(hc.small_window_cases()))


def test_emulated_limit_cases(http_main, tmp_path):
    """The 256 KiB limit: the final LF at 262143 and at 262144, no terminator at
    either length."""
    cases = list(hc.big_window_cases())
    assert len(cases) == 5
    _both(http_main, tmp_path, cases)


def test_emulated_fuzz_cases(http_main, tmp_path):
    _both(http_main, tmp_path, list(hc.fuzz_cases()))


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_emulated_name_stride(http_main, tmp_path, delta):
    """name_stride one below, at and one above a 5-byte name, next to shorter and
    longer ones; a row that is too small stays untouched."""
    by_name = dict(hc.lattice_cases())
    cases = [(n, by_name[n]) for n in hc.STRIDE_CASES]
    stride = 5 + delta
    exp = hc.expected(cases, http_ref.http_request_host, stride)
    assert [e[0] for e in exp] == [http_ref.NAME_CAP, 0, 0, 0, http_ref.NAME_CAP if delta < 0 else 0]
    _both(http_main, tmp_path, cases, stride)


def test_emulated_mixed_batch(http_main, tmp_path):
    """HTTP, TLS-record and unrecognised prefixes interleaved: every item as the
    restatement says, and every TLS item equal to what
    hyobfs_tls_record_sni_batch leaves on the same bytes."""
    cases = list(hc.mixed_cases())
    lines = _run(http_main, tmp_path, 2, [m for _, m in cases])
    exp = hc.expected(cases, http_ref.tcp_sniff)
    _check([n for n, _ in cases], exp, lines)
    tls = 0
    for (name, m), line in zip(cases, lines):
        f = line.split()
        if sni_ref.is_tls(m):
            assert f[:5] == f[5:], name
            tls += 1
        else:
            assert int(f[5]) == sni_ref.NOT_TLS, name
    kinds = collections.Counter(e[0] for e in exp)
    assert tls >= 80 and kinds[http_ref.UNRECOGNIZED] >= 8 and kinds[0] >= 100, (tls, kinds)
    # the four waves of some workgroup take three different branches
    groups = [tuple("h" if http_ref.is_http(m) else "t" if sni_ref.is_tls(m) else "u" for _, m in cases[g:g + 4])
              for g in range(0, len(cases) - 3, 4)]
    assert any(len(set(g)) == 3 for g in groups)


# ------------------------------------------------------------------ the Python surface without a GPU
def test_library_has_the_http_entry_points():
    from hysteria_amd import sniff
    lib = sniff._slib()
    # n == 0 is OK before any pointer is looked at; a null required pointer is INVALID
    assert lib.hyobfs_http_request_host_batch(None, None, None, 0, None, 0, None, None) == 0
    assert lib.hyobfs_tcp_sniff_batch(None, None, None, 0, None, 0, None, None) == 0
    assert lib.hyobfs_http_request_host_batch(None, None, None, 1, None, 0, None, None) == -2
    assert lib.hyobfs_tcp_sniff_batch(None, None, None, 1, None, 0, None, None) == -2


def test_statuses_match_header(tmp_path):
    from hysteria_amd import sniff
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hyobfs_sniff.h"\n#include "hyobfs_acl.h"\nint main(void){'
                   + "".join(f'printf("%d\\n", HYOBFS_SNIFF_ERR_{n});' for n in ("NOT_HTTP", "HOST", "UNRECOGNIZED"))
                   + 'printf("%d\\n", HYOBFS_ACL_ERR_PATTERN);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[:3] == [sniff.ERR_NOT_HTTP, sniff.ERR_HOST, sniff.ERR_UNRECOGNIZED] == [-65, -66, -67]
    assert vals[:3] == [http_ref.NOT_HTTP, http_ref.HOST, http_ref.UNRECOGNIZED]
    assert vals[3] == -64                                  # the new statuses continue after the ACL's
    assert all(s in sniff.ERRORS for s in vals[:3])
    assert sniff.MAX_HTTP_HEADER_BYTES == http_ref.MAX_HEADER_BYTES


def test_tcp_many_rewrites_addresses(monkeypatch):
    """Sniffer.tcp_many on mocked results: Check first, then a name rewrites the
    host and keeps the port; no name, HOST and every other status keep the address."""
    from hysteria_amd import sniff
    from hysteria_amd.sniff import Sniffer, SniffError
    seen = []

    def fake(prefixes, device=0, name_stride=sniff.MAX_NAME_LEN):
        seen.append(list(prefixes))
        table = {b"a": b"example.com", b"b": b"", b"c": SniffError(sniff.ERR_HOST), b"d": SniffError(sniff.ERR_MALFORMED),
                 b"e": SniffError(sniff.ERR_UNRECOGNIZED), b"f": b"2001:db8::1", b"g": SniffError(sniff.ERR_NEED_MORE)}
        return [table[p] for p in prefixes]

    monkeypatch.setattr(sniff, "tcp_snis", fake)
    s = Sniffer(rewrite_domain=False, tcp_ports=[(80, 80), (8080, 8080)])
    got = s.tcp_many([b"a", b"a", b"a", b"b", b"c", b"d", b"e", b"f", b"g", b"a"],
                     ["1.1.1.1:80", "example.org:80", "1.1.1.1:443", "2.2.2.2:80", "3.3.3.3:80", "4.4.4.4:8080",
                      "5.5.5.5:80", "[::1]:8080", "6.6.6.6:80", "@internal"])
    assert got == ["example.com:80", "example.org:80", "1.1.1.1:443", "2.2.2.2:80", "3.3.3.3:80", "4.4.4.4:8080",
                   "5.5.5.5:80", "[2001:db8::1]:8080", "6.6.6.6:80", "@internal"]
    assert seen == [[b"a", b"b", b"c", b"d", b"e", b"f", b"g"]]   # only what Check lets through is sniffed
    with pytest.raises(ValueError):
        s.tcp_many([b"a"], [])


def test_package_exports_http():
    import hysteria_amd
    for name in ("http_request_host_batch", "tcp_sniff_batch", "Sniffer", "sniff"):
        assert name in hysteria_amd.__all__ and hasattr(hysteria_amd, name)
    for name in ("http_request_hosts", "tcp_snis", "ERR_NOT_HTTP", "ERR_HOST", "ERR_UNRECOGNIZED"):
        assert hasattr(hysteria_amd.sniff, name)
    assert hasattr(hysteria_amd.Sniffer, "tcp_many") and hasattr(hysteria_amd.Sniffer, "tls_many")
