"""The UDP relay message kernels on the GPU (hysteria_amd/csrc/udpmsg.hip,
include/hyobfs_udpmsg.h): every case family of tests/udpmsg_cases.py through the
three device calls, bit-exact against the restatement (tests/udpmsg_ref.py), with
guard bytes around every output array; the round trip frag -> parse -> host
Defragger -> assemble; and the chain frag -> relay_quic_snis over client
Initials."""
import numpy as np
import pytest

import sni_ref
import sniff_cases as sc
import udpmsg_cases as uc
import udpmsg_ref as R
from test_udpmsg import assemble_inputs, check_assemble_result, check_send_result

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PAD = 64   # guard bytes (0xA5) on both sides of every output array


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _t(dev, a):
    return torch.from_numpy(np.array(a, copy=True)).to(dev)   # a writable copy


class Guarded:
    """nbytes of device memory between two runs of PAD guard bytes; the payload starts
    `mis` bytes past a 16-byte boundary."""

    def __init__(self, dev, nbytes, mis=0):
        self.lead, self.nbytes = PAD + mis, nbytes   # torch allocations are at least 256-aligned
        self.t = torch.full((self.lead + nbytes + PAD,), uc.GUARD, dtype=torch.uint8, device=dev)
        assert self.t.data_ptr() % 16 == 0 and PAD % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr() + self.lead

    def read(self, dtype=np.uint8):
        """The payload, after checking that both guards are intact."""
        h = self.t.cpu().numpy()
        assert (h[:self.lead] == uc.GUARD).all() and (h[self.lead + self.nbytes:] == uc.GUARD).all(), "guard bytes"
        return np.frombuffer(h[self.lead:self.lead + self.nbytes].tobytes(), dtype)


def send_inputs(dev, msgs):
    from hysteria_amd import udpmsg
    addrs, where = bytearray(), {}
    for m in msgs:
        if m[2] not in where:
            where[m[2]] = len(addrs)
            addrs += m[2]
    meta = np.zeros(len(msgs), udpmsg.META_DTYPE)
    for i, (sid, pid, addr, data, max_size) in enumerate(msgs):
        meta[i] = (sid, pid, 0, max_size, len(addr), where[addr])
    data, off, lens = uc.pack([m[3] for m in msgs])
    if data.size == 0:
        data = np.zeros(1, np.uint8)
    return (_t(dev, data), _t(dev, off), _t(dev, lens), _t(dev, meta.view(np.uint8)),
            _t(dev, np.frombuffer(bytes(addrs), np.uint8).copy()))


def run_send(dev, case):
    """hyobfs_udp_frag_batch over one case, every output between guards: the arguments of check_send_result."""
    from hysteria_amd import _lib, udpmsg
    n = len(case["msgs"])
    _, _, _, _, _, oc, dc = uc.expected_send(case)
    d_data, d_off, d_len, d_meta, d_addrs = send_inputs(dev, case["msgs"])
    out, status, first = Guarded(dev, oc, case["out_mis"]), Guarded(dev, 4 * n), Guarded(dev, 8 * (n + 1))
    totals, dgram_off, dgram_len = Guarded(dev, 16), Guarded(dev, 8 * dc), Guarded(dev, 4 * dc)
    ws = Guarded(dev, udpmsg.frag_workspace_size(n))
    rc = udpmsg._ulib().hyobfs_udp_frag_batch(
        d_data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), d_meta.data_ptr(), d_addrs.data_ptr(), n,
        out.ptr if oc else None, oc, dgram_off.ptr if dc else None, dgram_len.ptr if dc else None, dc, first.ptr,
        status.ptr, totals.ptr, ws.ptr, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    ws.read()
    return (rc, status.read(np.int32), first.read(np.uint64), totals.read(np.uint64), dgram_off.read(np.uint64),
            dgram_len.read(np.uint32), b"", out.read())


def _names(cases):
    return [c["name"] for c in cases]


@pytest.mark.parametrize("case", uc.lattice_cases() + uc.capacity_cases() + uc.scan_cases(),
                         ids=_names(uc.lattice_cases() + uc.capacity_cases() + uc.scan_cases()))
def test_frag_batch_families(dev, case):
    check_send_result(case, *run_send(dev, case))


def test_lattice_residues():
    src, dst = uc.residues(uc.lattice_msgs())
    assert src == set(range(16)) and dst == set(range(16))


def _parse(dev, items):
    from hysteria_amd import udpmsg
    buf, off, lens = uc.pack(items)
    d_in, d_off = _t(dev, np.concatenate([buf, np.zeros(1, np.uint8)])), _t(dev, off)
    out = Guarded(dev, 32 * len(items))
    udpmsg.parse_batch(d_in, d_off, _t(dev, lens), len(items), out.ptr, torch.cuda.current_stream(dev))
    torch.cuda.synchronize(dev)
    return d_in, d_off, out


def test_parse_batch_family(dev):
    from hysteria_amd import udpmsg
    items = uc.parse_datagrams()
    uc.truncation_coverage(uc.produced_datagrams(), items)   # every produced datagram, see parse_datagrams()
    got = _parse(dev, items)[2].read(udpmsg.PARSED_DTYPE)
    want = np.array([R.parsed_record(d) + (0,) for d in items], udpmsg.PARSED_DTYPE)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (int(bad[0]), items[int(bad[0])][:24].hex(), got[bad[0]], want[bad[0]])
    assert set(want["status"].tolist()) == {R.OK, R.TRUNCATED, R.ADDR_LEN, R.MSG_LEN}


def _assemble(dev, d_in, d_off, d_parsed_ptr, n, lists, caps, gaps):
    from hysteria_amd import udpmsg
    m = len(lists)
    idx = np.array([i for l in lists for i in l] or [0], np.uint32)
    first = np.zeros(m + 1, np.uint64)
    np.cumsum([len(l) for l in lists], out=first[1:])
    out_off, total = np.zeros(m, np.uint64), 0
    for j in range(m):
        total += gaps[j]
        out_off[j] = total
        total += caps[j]
    out, out_len, status = Guarded(dev, total, 7), Guarded(dev, 4 * m), Guarded(dev, 4 * m)
    udpmsg.assemble_batch(d_in, d_off, d_parsed_ptr, n, _t(dev, idx), _t(dev, first), m, out.ptr, _t(dev, out_off),
                          _t(dev, np.array(caps, np.uint32)), out_len.ptr, status.ptr, torch.cuda.current_stream(dev))
    torch.cuda.synchronize(dev)
    return status.read(np.int32), out_len.read(np.uint32), out.read(), out_off


def test_assemble_batch_family(dev):
    stream, lists, caps, gaps, exp_st, want = assemble_inputs()
    d_in, d_off, parsed = _parse(dev, stream)
    status, out_len, out, _ = _assemble(dev, d_in, d_off, parsed.ptr, len(stream), lists, caps, gaps)
    check_assemble_result(status, out_len, out, caps, gaps, exp_st, want)


def test_round_trip_random(dev):
    """frag_batch -> parse_batch -> the host Defragger -> assemble_batch gives back every message's data."""
    from hysteria_amd import udpmsg
    case = uc.random_case()
    msgs = case["msgs"]
    res = run_send(dev, case)
    check_send_result(case, *res)
    dgram_off, dgram_len, out = res[4], res[5], res[7]
    assert len(dgram_off) > len(msgs)   # the 1350-byte half is fragmented
    d_in = _t(dev, np.concatenate([out, np.zeros(1, np.uint8)]))
    d_off = _t(dev, dgram_off)
    parsed = Guarded(dev, 32 * len(dgram_off))
    udpmsg.parse_batch(d_in, d_off, _t(dev, dgram_len), len(dgram_off), parsed.ptr, torch.cuda.current_stream(dev))
    torch.cuda.synchronize(dev)
    recs = parsed.read(udpmsg.PARSED_DTYPE)
    assert (recs["status"] == 0).all()
    # one Defragger per message here: the random session ids of this family are not sessions
    lists = []
    for i, st in enumerate(res[2][:-1]):
        d = udpmsg.Defragger()
        for k in range(int(st), int(res[2][i + 1])):
            state, tags = d.feed(recs[k], k)
        assert state in (udpmsg.WHOLE, udpmsg.COMPLETE)
        lists.append(tags)
        d.close()
    caps = [len(m[3]) for m in msgs]
    status, out_len, back, out_off = _assemble(dev, d_in, d_off, parsed.ptr, len(dgram_off), lists, caps,
                                               [j % 5 for j in range(len(msgs))])
    assert (status == 0).all() and out_len.tolist() == caps
    for j, m in enumerate(msgs):
        assert back[int(out_off[j]):int(out_off[j]) + caps[j]].tobytes() == m[3], j


def test_chain_relayed_initials_to_server_names(dev):
    """Client Initials wrapped as relay messages with max_size 1200 go through frag_batch
    and come back through relay_quic_snis: every server name comes out."""
    import quic_cases as qc
    from hysteria_amd import udpmsg
    from oracle import quic_ref as ref
    hellos = [m for _, m in sc.generator_cases() if sni_ref.client_hello_sni(m)[0] == 0 and sni_ref.client_hello_sni(m)[1]]
    hellos = hellos[:48]
    assert len(hellos) >= 16
    pkts, want = [], []
    for k, msg in enumerate(hellos):
        if k % 2:   # padded to a full-size Initial, as clients send them
            frames = qc._crypto(0, msg)
            frames += b"\x00" * max(0, 1200 - len(frames))
            pkt = ref.client_initial(bytes((k + j) & 0xFF for j in range(8)), b"", ref.V1, b"", 2, 2, frames)
            assert len(pkt) >= 1200
        else:
            pkt = sc.initial_for(msg, k)
        pkts.append(pkt)
        want.append(sni_ref.client_hello_sni(msg)[4])
    msgs = [(1000 + k, 1 + k, b"198.51.100.7:443", p, 1200) for k, p in enumerate(pkts)]
    assert all(R.send(*m)[0] == R.OK for m in msgs)
    case = dict(name="chain", msgs=msgs, out_cap=None, dgram_cap=None, out_mis=0)
    res = run_send(dev, case)
    check_send_result(case, *res)
    first, dgram_off, dgram_len, out = res[2], res[4], res[5], res[7]
    assert any(int(first[i + 1] - first[i]) > 1 for i in range(len(msgs)))   # at least one Initial really was fragmented
    dgrams = [out[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(dgram_off, dgram_len)]
    # sessions interleaved: all first fragments, then the rest in reverse
    order = [int(first[i]) for i in range(len(msgs))]
    order += [d for d in reversed(range(len(dgrams))) if d not in set(order)]
    got = udpmsg.relay_quic_snis([dgrams[d] for d in order], device=dev.index or 0)
    # completion order: whole messages as their only datagram arrives, fragmented ones in the second part
    done = [i for i in range(len(msgs)) if first[i + 1] - first[i] == 1]
    done += [i for i in reversed(range(len(msgs))) if first[i + 1] - first[i] > 1]
    assert got == [want[i] for i in done]
