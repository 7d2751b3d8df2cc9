"""The sniffer's server-name extraction on the GPU (hysteria_amd/csrc/sniff.hip,
include/hyobfs_sniff.h) against the restatement of its rules (tests/sni_ref.py,
pinned in tests/test_sniff.py to sniff_test.go:86,135)."""
import base64
import json
import os

import numpy as np
import pytest

import quic_cases as qc
import sni_ref
import sniff_cases as sc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(ROOT, "tests", "golden", "sniff_vectors.json")) as f:
        return json.load(f)


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _sres(t):
    from hysteria_amd import sniff
    return np.frombuffer(t.cpu().numpy().tobytes(), sniff.SNIFF_RESULT_DTYPE)


def _sni(dev, call, msgs, stride=sc.NAME_STRIDE):
    """One batched call over pack(msgs, gap 3): (records, names as [n, stride])."""
    buf, off, lens = sc.pack(msgs, gap=3)
    n = len(msgs)
    d_names = torch.full((n * stride + 64,), sc.SENTINEL, dtype=torch.uint8, device=dev)
    d_res = torch.full((n * 16,), 0xFF, dtype=torch.uint8, device=dev)
    call(_t(dev, buf), _t(dev, off), _t(dev, lens), n, d_names, stride, d_res)
    names = d_names.cpu().numpy()
    assert (names[n * stride:] == sc.SENTINEL).all()
    return _sres(d_res), names[:n * stride].reshape(n, stride)


def _check(labels, exp, res, names):
    """status, name_len, name_off, need, the name bytes and the sentinel everywhere
    else in `names`, per message."""
    stride = names.shape[1]
    assert len(res) == len(exp) == len(names)
    for i, (label, e) in enumerate(zip(labels, exp)):
        r = res[i]
        got = (int(r["status"]), int(r["name_len"]), int(r["name_off"]), int(r["need"]))
        assert got == e[:4], (label, got, e[:4])
        want = e[4] + bytes([sc.SENTINEL]) * (stride - len(e[4]))
        assert names[i].tobytes() == want, label


def test_client_hello_cases(dev):
    """Every generator, window-boundary and fuzz case through
    hyobfs_tls_client_hello_sni_batch."""
    from hysteria_amd import sniff
    cases = sc.all_cases()
    res, names = _sni(dev, sniff.client_hello_sni_batch, [m for _, m in cases])
    _check([n for n, _ in cases], sc.expected(cases, sni_ref.client_hello_sni), res, names)


def test_tls_record_cases(dev):
    """The same cases as TLS record bodies, and the record layer's own cases
    (isTLS, NEED_MORE, a stream that goes on), through hyobfs_tls_record_sni_batch."""
    from hysteria_amd import sniff
    cases = list(sc.record_cases())
    res, names = _sni(dev, sniff.tls_record_sni_batch, [m for _, m in cases])
    _check([n for n, _ in cases], sc.expected(cases, sni_ref.tls_record_sni), res, names)


def _quic_sniff(dev, pkts, cap=2048, stride=sc.NAME_STRIDE):
    """quic_sniff_batch over pack(pkts), and read_crypto_payload_batch alone on a
    copy of the same input: ((sres, names), (qres, crypto, packets) of each call)."""
    from hysteria_amd import quic, sniff
    n = len(pkts)
    buf, off, lens = qc.pack(pkts)
    d_off, d_len = _t(dev, off), _t(dev, lens)
    d_coff = _t(dev, np.arange(n, dtype=np.uint64) * np.uint64(cap))
    d_cap = _t(dev, np.full(n, cap, np.uint32))
    d_names = torch.full((n * stride + 64,), sc.SENTINEL, dtype=torch.uint8, device=dev)
    d_sres = torch.full((n * 16,), 0xFF, dtype=torch.uint8, device=dev)
    outs = []
    for fused in (True, False):
        d_buf = _t(dev, buf)
        d_crypto = torch.full((n * cap + 64,), sc.SENTINEL, dtype=torch.uint8, device=dev)
        d_qres = torch.zeros(n * 24, dtype=torch.uint8, device=dev)
        if fused:
            ws = torch.empty(sniff.quic_sniff_workspace_size(n), dtype=torch.uint8, device=dev)
            sniff.quic_sniff_batch(d_buf, d_off, d_len, n, d_crypto, d_coff, d_cap, d_qres, d_names, stride, d_sres,
                                   ws)
        else:
            ws = torch.empty(quic.workspace_size(n), dtype=torch.uint8, device=dev)
            quic.read_crypto_payload_batch(d_buf, d_off, d_len, n, d_crypto, d_coff, d_cap, d_qres, ws)
        outs.append((d_qres.cpu().numpy(), d_crypto.cpu().numpy(), d_buf.cpu().numpy()))
    names = d_names.cpu().numpy()
    assert (names[n * stride:] == sc.SENTINEL).all()
    return (_sres(d_sres), names[:n * stride].reshape(n, stride)), outs[0], outs[1]


def test_quic_sniff_cases(dev):
    """hyobfs_quic_sniff_batch over client Initials holding every case, then
    quic_cases.crypto_packets(): failed packets are NO_PAYLOAD, random payloads
    MALFORMED or NOT_HELLO as the restatement says, and qres, crypto and the
    packets are byte-equal to a plain read_crypto_payload_batch call's."""
    from hysteria_amd import quic
    cases = list(sc.quic_cases(True))
    (res, names), fused, plain = _quic_sniff(dev, [p for _, p, _ in cases])
    exp = sc.expected_quic(cases)
    _check([n for n, _, _ in cases], exp, res, names)
    for a, b, what in zip(fused, plain, ("qres", "crypto", "packets")):
        assert np.array_equal(a, b), what
    qres = np.frombuffer(fused[0].tobytes(), quic.RESULT_DTYPE)
    rnd = {"NO_PAYLOAD": 0, "other": 0}
    for i, (name, _, payload) in enumerate(cases):
        assert (int(qres[i]["status"]) == 0) == (payload is not None), name
        if name.startswith("quic_pkt_"):
            st = int(res[i]["status"])
            if payload is None:
                assert st == sni_ref.NO_PAYLOAD, name
                rnd["NO_PAYLOAD"] += 1
            else:
                assert st in (sni_ref.MALFORMED, sni_ref.NOT_HELLO), (name, st)
                rnd["other"] += 1
    assert rnd["NO_PAYLOAD"] >= 10 and rnd["other"] >= 10, rnd


def test_reference_vectors_through_sniffer(dev, vectors):
    """TestSnifferTCP's TLS input and TestSnifferUDP's Initial (sniff_test.go:86-93,
    :133-139) through Sniffer.tls_many / Sniffer.udp_many, next to inputs the
    sniffer must leave alone."""
    from hysteria_amd import Sniffer
    s = Sniffer(timeout=1.0, rewrite_domain=False)
    t, q = vectors["tls_record"], vectors["quic_initial"]
    tls, pkt = base64.b64decode(t["data_b64"]), base64.b64decode(q["data_b64"])
    got = s.tls_many([tls, b"Wait It's All Ohio? Always Has Been.", tls, tls[:100], tls, tls],
                     [t["req_addr"], "123.123.123.123:123", "example.com:443", "7.7.7.7:443", "[2001:db8::1]:8443",
                      "@internal"])
    assert got == [t["rewritten"], "123.123.123.123:123", "example.com:443", "7.7.7.7:443", "ipinfo.io:8443",
                   "@internal"]
    bad = bytearray(pkt)
    bad[-1] ^= 1
    got = s.udp_many([pkt, bytes(bad), pkt, b"\x01\x02\x03", pkt], [q["req_addr"], "2.3.4.5:443", "notion.so:443",
                                                                    "8.8.8.8:53", "[::1]:443"])
    assert got == [q["rewritten"], "2.3.4.5:443", "notion.so:443", "8.8.8.8:53", "www.notion.so:443"]
    assert Sniffer(rewrite_domain=True, udp_ports=[(443, 443)]).udp_many([pkt, pkt], ["notion.so:443", "1.1.1.1:80"]) \
        == ["www.notion.so:443", "1.1.1.1:80"]
    assert s.udp_many([], []) == [] and s.tls_many([], []) == []


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes(dev, n):
    """Batches of 1, 63, 64 and 65 messages (a partial group of four, 16 groups,
    one message past them) through the three entry points, name_stride 64 so
    that longer names are NAME_CAP."""
    from hysteria_amd import sniff
    allc = sc.all_cases()
    cases = [allc[(5 + 11 * k) % len(allc)] for k in range(n)]
    res, names = _sni(dev, sniff.client_hello_sni_batch, [m for _, m in cases], 64)
    _check([c[0] for c in cases], sc.expected(cases, sni_ref.client_hello_sni, 64), res, names)
    recs = [(c[0], sc.as_record(c[1])) for c in cases]
    res, names = _sni(dev, sniff.tls_record_sni_batch, [m for _, m in recs], 64)
    _check([c[0] for c in recs], sc.expected(recs, sni_ref.tls_record_sni, 64), res, names)
    quic = [sc.quic_cases(True)[(5 + 11 * k) % len(allc)] for k in range(n)]
    (res, names), fused, plain = _quic_sniff(dev, [p for _, p, _ in quic], stride=64)
    _check([c[0] for c in quic], sc.expected_quic(quic, 64), res, names)
    for a, b in zip(fused, plain):
        assert np.array_equal(a, b)


def test_batch_above_the_grid_cap(dev):
    """More messages than one pass of the grid takes (65536 workgroups of four):
    minimal hellos of 45 to 64 bytes, so every wave takes a second message of
    another kind and the last group of the second pass is partial."""
    from hysteria_amd import sniff
    temps = sc.small_templates()
    exp_t = [sni_ref.client_hello_sni(t, 4) for t in temps]
    assert {e[0] for e in exp_t} == {0, sni_ref.MALFORMED, sni_ref.NOT_HELLO}
    n = sc.GRID_CAP_MSGS + 259
    rng = np.random.default_rng(41)
    pick = rng.integers(0, len(temps), n)
    second = np.arange(sc.GRID_CAP_MSGS, n)
    pick[second] = (pick[second - sc.GRID_CAP_MSGS] + 1 + rng.integers(0, len(temps) - 1, len(second))) % len(temps)
    assert (pick[second] != pick[second - sc.GRID_CAP_MSGS]).all()
    slot = 64
    rows = np.full((len(temps), slot), sc.SENTINEL, np.uint8)
    for k, t in enumerate(temps):
        rows[k, :len(t)] = np.frombuffer(t, np.uint8)
    stride = 4
    d_names = torch.full((n * stride,), sc.SENTINEL, dtype=torch.uint8, device=dev)
    d_res = torch.full((n * 16,), 0xFF, dtype=torch.uint8, device=dev)
    sniff.client_hello_sni_batch(_t(dev, rows[pick].reshape(-1)), _t(dev, np.arange(n, dtype=np.uint64) * np.uint64(slot)),
                                 _t(dev, np.array([len(t) for t in temps], np.uint32)[pick]), n, d_names, stride, d_res)
    res = _sres(d_res)
    for j, f in enumerate(("status", "name_len", "name_off", "need")):
        want = np.array([e[j] for e in exp_t])[pick]
        bad = np.nonzero(res[f] != want)[0]
        assert not len(bad), (f, int(bad[0]), int(pick[bad[0]]))
    want_rows = np.full((len(temps), stride), sc.SENTINEL, np.uint8)
    for k, e in enumerate(exp_t):
        want_rows[k, :len(e[4])] = np.frombuffer(e[4], np.uint8)
    got = d_names.cpu().numpy().reshape(n, stride)
    bad = np.nonzero((got != want_rows[pick]).any(axis=1))[0]
    assert not len(bad), ("names", int(bad[0]), int(pick[bad[0]]))


def test_helpers(dev):
    """client_hello_snis / tls_record_snis / quic_snis: bytes or a SniffError per item."""
    from hysteria_amd import sniff
    by_name = dict(sc.generator_cases())
    got = sniff.client_hello_snis([by_name["valid"], by_name["no_type_0"], by_name["trailing_dot"], by_name["len_2"]])
    assert got[:2] == [b"example.org", b""]
    assert [g.status for g in got[2:]] == [sniff.ERR_MALFORMED, sniff.ERR_NOT_HELLO]
    got = sniff.tls_record_snis([sc.as_record(by_name["valid"]), sc.as_record(by_name["valid"])[:40], b"GET / HTTP/1.1"])
    assert got[0] == b"example.org" and [g.status for g in got[1:]] == [sniff.ERR_NEED_MORE, sniff.ERR_NOT_TLS]
    # a payload past crypto_cap is read again with the reference's limit
    got = sniff.quic_snis([sc.initial_for(by_name["extensions_256"], 0), sc.initial_for(by_name["valid"], 1), b"\x00"],
                          crypto_cap=512)
    assert got[:2] == [b"example.org", b"example.org"] and got[2].status == sniff.ERR_NO_PAYLOAD
