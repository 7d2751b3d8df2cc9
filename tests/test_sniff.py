"""CPU tier of the sniffer's server-name extraction (include/hyobfs_sniff.h):
the Python restatement (tests/sni_ref.py) against the reference's own vectors,
the kernel itself through a stand-alone AddressSanitizer build (tests/emu/
sniff_main.cpp + sniff.hip + quic.hip against hip_emu.h, run as a child
process), Sniffer.check against TestSnifferCheck (sniff_test.go:15-36) and the
request-address rewriting."""
import base64
import collections
import fcntl
import json
import os
import struct
import subprocess

import pytest

import sni_ref
import sniff_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(ROOT, "tests", "golden", "sniff_vectors.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------ the restatement
def test_restatement_reference_tls_vector(vectors):
    """sniff_test.go:86-93: the record's ClientHello names ipinfo.io."""
    v = vectors["tls_record"]
    data = base64.b64decode(v["data_b64"])
    st, name_len, name_off, need, name = sni_ref.tls_record_sni(data)
    assert (st, name, need) == (0, v["server_name"].encode(), 0)
    assert data[name_off:name_off + name_len] == name
    # the record's body alone is a handshake message of type 1
    assert sni_ref.client_hello_sni(data[5:])[4] == name
    assert sni_ref.tls_record_sni(data[:-1])[:4] == (sni_ref.NEED_MORE, 0, 0, len(data))


def test_restatement_reference_quic_vector(vectors):
    """sniff_test.go:133-139: the Initial's CRYPTO data (814 bytes by the QUIC
    oracle) names www.notion.so."""
    from oracle import quic_ref
    v = vectors["quic_initial"]
    payload = quic_ref.read_crypto_payload(base64.b64decode(v["data_b64"]))
    assert len(payload) == v["crypto_payload_len"] == 814
    st, name_len, name_off, _, name = sni_ref.client_hello_sni(payload)
    assert (st, name) == (0, v["server_name"].encode())
    assert payload[name_off:name_off + name_len] == name


def test_restatement_statuses_of_the_generator_cases():
    """Spot checks that pin the restatement's reading of the rules."""
    exp = {n: sni_ref.client_hello_sni(m, sc.NAME_STRIDE) for n, m in sc.generator_cases()}
    ok_name = [n for n, e in exp.items() if e[0] == 0 and e[1]]
    for n in ("valid", "wrong_uint24_length", "uint24_length_max", "no_cipher_suites", "extensions_256", "name_len_255",
              "host_after_other_entry", "inner_dot_only"):
        assert n in ok_name, n
    for n in ("no_extensions_block", "empty_extensions_block", "no_type_0", "only_non_host_entries"):
        assert exp[n][:3] == (0, 0, 0), n
    for n in ("trailing_dot", "two_host_names", "empty_name", "empty_name_list", "list_len_short", "list_len_long",
              "list_trailing_bytes", "odd_cipher_suites", "duplicate_type_0", "duplicate_other_type",
              "ext_header_truncated", "ext_body_truncated", "ext_block_shorter", "ext_block_longer",
              "trailing_after_extensions", "len_4", "extensions_256_dup_last", "name_len_256_then_dup"):
        assert exp[n][0] == sni_ref.MALFORMED, n
    for n in ("type_byte_2", "len_0", "len_1", "len_2", "len_3"):
        assert exp[n][0] == sni_ref.NOT_HELLO, n
    assert exp["name_len_256"][:3] == (sni_ref.NAME_CAP, 256, 104)
    assert exp["extensions_257"][0] == exp["extensions_257_sni_first"][0] == sni_ref.EXTENSIONS


def test_fuzz_set_is_balanced():
    """Of the 512 single-byte mutations at least a quarter stay OK with a name and
    at least a quarter become malformed, by the restatement alone."""
    cases = sc.fuzz_cases()
    assert len(cases) == 512
    kinds = collections.Counter((e[0], e[1] > 0) for e in sc.expected(cases, sni_ref.client_hello_sni))
    assert kinds[(0, True)] >= 128 and kinds[(sni_ref.MALFORMED, False)] >= 128, kinds


def test_window_cases_cover_the_edges():
    """The extensions length field, an extension header, the name-list header and
    the name each start at bytes 62, 63, 64 and 65 in some case."""
    hit = collections.defaultdict(set)
    for sid in range(33):
        for pad in range(80):
            name = f"window_sid{sid}_pad{pad}"
            if any(n == name for n, _ in sc.window_cases()):
                for f, p in sc._offsets(sid, pad)[1].items():
                    hit[f].add(p)
    for f in ("ext_len", "sni_hdr", "list_hdr", "name"):
        assert {62, 63, 64, 65} <= hit[f], (f, sorted(hit[f]))


# ------------------------------------------------------------------ the kernel on the CPU
@pytest.fixture(scope="module")
def sniff_main():
    """tests/emu/build/sniff_main: sniff.hip + quic.hip + the driver, compiled for
    the host with AddressSanitizer (a program with its own main: nothing is
    preloaded).  Rebuilt when a source is newer."""
    if not os.path.exists(CLANG):
        pytest.skip("no host clang for the emulated build")
    csrc = os.path.join(ROOT, "hysteria_amd", "csrc")
    srcs = [os.path.join(EMU, "sniff_main.cpp"), os.path.join(csrc, "sniff.hip"), os.path.join(csrc, "quic.hip")]
    deps = srcs + [os.path.join(EMU, "hip_emu.h"), os.path.join(csrc, "kernels.h"), os.path.join(csrc, "sha256.h"),
                   os.path.join(csrc, "quic_crypto.h"), os.path.join(ROOT, "include", "hyobfs_sniff.h"),
                   os.path.join(ROOT, "include", "hyobfs_quic.h")]
    os.makedirs(os.path.join(EMU, "build"), exist_ok=True)
    exe = os.path.join(EMU, "build", "sniff_main")
    with open(os.path.join(EMU, "build", ".sniff_main.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
            tmp = exe + ".tmp"
            subprocess.run([CLANG, "-std=c++20", "-O1", "-g", "-DHYOBFS_EMULATE", "-I" + EMU, "-I" + csrc, "-x", "c++",
                            "-fsanitize=address", "-fno-omit-frame-pointer", "-pthread",
                            "-Wno-unused-command-line-argument", *srcs, "-o", tmp], check=True, capture_output=True)
            os.replace(tmp, exe)
    return exe


def _run(exe, tmp_path, mode, msgs, stride=sc.NAME_STRIDE, cap=2048):
    path = tmp_path / f"cases{mode}.bin"
    path.write_bytes(struct.pack("<4I", mode, len(msgs), stride, cap)
                     + b"".join(struct.pack("<I", len(m)) + m for m in msgs))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "tail a5"
    return lines[:-1]


def _check(names, exp, lines, stride=sc.NAME_STRIDE):
    assert len(lines) >= len(exp)
    for name, e, line in zip(names, exp, lines):
        f = line.split()
        assert tuple(int(x) for x in f[:4]) == e[:4], (name, f[:4], e[:4])
        assert bytes.fromhex(f[4]) == e[4] + bytes([sc.SENTINEL]) * (stride - len(e[4])), name


def test_emulated_client_hello_cases(sniff_main, tmp_path):
    """Every generator, window and fuzz case through hyobfs_tls_client_hello_sni_batch
    under AddressSanitizer, the gaps between messages poisoned."""
    cases = sc.all_cases()
    lines = _run(sniff_main, tmp_path, 0, [m for _, m in cases])
    _check([n for n, _ in cases], sc.expected(cases, sni_ref.client_hello_sni), lines)


def test_emulated_tls_record_cases(sniff_main, tmp_path):
    """The record layer's cases and the generator and window cases as record
    bodies (the fuzz set has run above) through hyobfs_tls_record_sni_batch."""
    cases = [c for c in sc.record_cases() if not c[0].startswith("rec_fuzz")]
    assert len(cases) > 120
    lines = _run(sniff_main, tmp_path, 1, [m for _, m in cases])
    _check([n for n, _ in cases], sc.expected(cases, sni_ref.tls_record_sni), lines)


def test_emulated_quic_sniff_cases(sniff_main, tmp_path, vectors):
    """hyobfs_quic_sniff_batch over Initials holding the generator and window
    cases, good and bad Initials with random payloads, and the reference's
    vector; qres, crypto and the packets as read_crypto_payload_batch alone
    leaves them."""
    v = vectors["quic_initial"]
    cases = list(sc.quic_cases(False))
    lines = _run(sniff_main, tmp_path, 2, [p for _, p, _ in cases] + [base64.b64decode(v["data_b64"])])
    assert lines[-1] == "same 1"
    exp = sc.expected_quic(cases)
    _check([n for n, _, _ in cases], exp, lines)
    for (name, _, payload), line in zip(cases, lines):
        assert (int(line.split()[5]) == 0) == (payload is not None), name
    assert collections.Counter(e[0] for e in exp)[sni_ref.NO_PAYLOAD] >= 10
    f = lines[len(cases)].split()
    assert int(f[0]) == 0 and bytes.fromhex(f[4])[:int(f[1])] == v["server_name"].encode()


def test_emulated_small_stride_and_single_message(sniff_main, tmp_path):
    """name_stride 11: an 11-byte name fills its row, a 12-byte one is NAME_CAP
    and its row stays untouched; and a batch of one."""
    by_name = dict(sc.generator_cases())
    cases = [(n, by_name[n]) for n in ("valid", "inner_dot_only", "name_len_1", "no_type_0")]
    lines = _run(sniff_main, tmp_path, 0, [m for _, m in cases], stride=11)
    exp = sc.expected(cases, sni_ref.client_hello_sni, 11)
    assert [e[0] for e in exp] == [0, sni_ref.NAME_CAP, 0, 0]
    _check([n for n, _ in cases], exp, lines, 11)
    lines = _run(sniff_main, tmp_path, 1, [sc.record_cases()[0][1]])
    _check(["one"], sc.expected(sc.record_cases()[:1], sni_ref.tls_record_sni), lines)


# ------------------------------------------------------------------ the Python surface without a GPU
def test_library_has_the_sniff_entry_points():
    from hysteria_amd import sniff
    lib = sniff._slib()
    assert lib.hyobfs_quic_sniff_workspace_size(7) == lib.hyobfs_quic_workspace_size(7)
    # n == 0 is OK before any pointer is looked at; a null required pointer is INVALID
    assert lib.hyobfs_tls_client_hello_sni_batch(None, None, None, 0, None, 0, None, None) == 0
    assert lib.hyobfs_tls_record_sni_batch(None, None, None, 0, None, 0, None, None) == 0
    assert lib.hyobfs_quic_sniff_batch(None, None, None, 0, None, None, None, None, None, 0, None, None, None) == 0
    assert lib.hyobfs_tls_client_hello_sni_batch(None, None, None, 1, None, 0, None, None) == -2
    assert lib.hyobfs_tls_record_sni_batch(None, None, None, 1, None, 0, None, None) == -2
    assert lib.hyobfs_quic_sniff_batch(None, None, None, 1, None, None, None, None, None, 0, None, None, None) == -2


def test_result_record_matches_header(tmp_path):
    from hysteria_amd import sniff
    src = tmp_path / "probe.c"
    body = "\n".join(f'printf("%zu\\n", offsetof(hyobfs_sniff_result, {c}));' for c in sniff.SNIFF_RESULT_DTYPE.names)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hyobfs_sniff.h"\nint main(void){\n' + body
                   + '\nprintf("%zu\\n", sizeof(hyobfs_sniff_result));'
                   + "".join(f'\nprintf("%d\\n", HYOBFS_SNIFF_ERR_{n});' for n in
                             ("NOT_HELLO", "MALFORMED", "NAME_CAP", "EXTENSIONS", "NOT_TLS", "NEED_MORE", "NO_PAYLOAD"))
                   + '\nprintf("%d\\n", HYOBFS_TLS_MAX_EXTENSIONS);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt = sniff.SNIFF_RESULT_DTYPE
    assert vals[:5] == [dt.fields[n][1] for n in dt.names] + [dt.itemsize]
    assert vals[5:12] == [sniff.ERR_NOT_HELLO, sniff.ERR_MALFORMED, sniff.ERR_NAME_CAP, sniff.ERR_EXTENSIONS,
                          sniff.ERR_NOT_TLS, sniff.ERR_NEED_MORE, sniff.ERR_NO_PAYLOAD]
    assert vals[5:12] == [sni_ref.NOT_HELLO, sni_ref.MALFORMED, sni_ref.NAME_CAP, sni_ref.EXTENSIONS, sni_ref.NOT_TLS,
                          sni_ref.NEED_MORE, sni_ref.NO_PAYLOAD]
    assert vals[12] == sniff.MAX_EXTENSIONS == sni_ref.MAX_EXTENSIONS


def test_sniffer_check():
    """TestSnifferCheck (sniff_test.go:15-36)."""
    from hysteria_amd import Sniffer
    s = Sniffer(timeout=1.0, rewrite_domain=False, tcp_ports=None, udp_ports=None)
    assert s.check(False, "1.1.1.1:80")
    assert not s.check(False, "example.com:443")
    s.rewrite_domain = True
    assert s.check(False, "example.com:443")
    s.tcp_ports = [(80, 80)]
    assert s.check(False, "google.com:80")
    assert not s.check(False, "google.com:443")
    s.udp_ports = [(443, 443)]
    assert s.check(True, "google.com:443")
    assert not s.check(True, "google.com:80")


def test_sniffer_check_addresses():
    """Check's other returns (sniff.go:68-82): internal addresses, addresses
    SplitHostPort refuses, ports Atoi refuses, bracketed IPv6."""
    from hysteria_amd import Sniffer
    s = Sniffer()
    assert not s.check(False, "@speedtest")
    assert not s.check(True, "1.1.1.1")            # missing port
    assert not s.check(True, "::1:443")            # too many colons
    assert not s.check(True, "1.1.1.1:https")
    assert not s.check(True, "1.1.1.1: 443")
    assert s.check(True, "[2001:db8::1]:443")
    assert s.check(False, "[::ffff:1.2.3.4]:80")
    assert not s.check(False, "[example.com]:80")  # a domain, rewriting disabled
    assert not s.check(False, "[fe80::1%eth0]:80")  # ParseIP takes no zone
    assert Sniffer(udp_ports=[(1000, 2000), (443, 443)]).check(True, "9.9.9.9:1500")
    assert not Sniffer(udp_ports=[]).check(True, "9.9.9.9:1500")


def test_address_rewriting():
    """SplitHostPort / JoinHostPort as Sniffer.UDP uses them (sniff.go:166-171):
    the port is kept, a host holding ':' or '%' gets brackets."""
    from hysteria_amd.sniff import Sniffer, SniffError, join_host_port, split_host_port
    assert split_host_port("2.3.4.5:443") == ("2.3.4.5", "443")
    assert split_host_port("[2001:db8::1]:8443") == ("2001:db8::1", "8443")
    assert split_host_port("example.com:80") == ("example.com", "80")
    assert split_host_port(":80") == ("", "80") and split_host_port("host:") == ("host", "")
    for bad in ("2.3.4.5", "2001:db8::1", "[::1]", "[::1]443", "[::1]:4:3", "[::1:443", "a[b]:1", "::1]:443",
                "[::1]x:443"):
        with pytest.raises(ValueError):
            split_host_port(bad)
    assert join_host_port("www.notion.so", "443") == "www.notion.so:443"
    assert join_host_port("2001:db8::1", "443") == "[2001:db8::1]:443"
    assert join_host_port("fe80::1%eth0", "53") == "[fe80::1%eth0]:53"
    assert Sniffer._rewrite("2.3.4.5:443", b"www.notion.so") == "www.notion.so:443"
    assert Sniffer._rewrite("[2001:db8::1]:8443", b"ipinfo.io") == "ipinfo.io:8443"
    assert Sniffer._rewrite("example.com:80", b"other.example") == "other.example:80"
    assert Sniffer._rewrite("2.3.4.5:443", b"") == "2.3.4.5:443"                      # a hello without a name
    assert Sniffer._rewrite("2.3.4.5:443", SniffError(-55)) == "2.3.4.5:443"          # no hello at all
    assert Sniffer._rewrite("2.3.4.5:443", b"a:b") == "[a:b]:443"


def test_package_exports():
    import hysteria_amd
    for name in ("Sniffer", "SniffError", "SNIFF_RESULT_DTYPE", "client_hello_sni_batch", "tls_record_sni_batch",
                 "quic_sniff_batch", "sniff"):
        assert name in hysteria_amd.__all__ and hasattr(hysteria_amd, name)
