"""Realm punch matcher on the GPU (hyobfs_punch_match_batch, punch_conn.go:146-165):
every datagram against every registered attempt, vs the hashlib restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import realm_ref as rref  # noqa: E402
import wire_cases as wc  # noqa: E402
from punch_cases import punch_batch  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,m,seed", [(1, 1, 1), (5000, 1, 2), (20000, 6, 3), (3000, 32, 4)])
def test_match_batch_vs_oracle(gpu, n, m, seed):
    import torch
    from hysteria_amd import realm
    pk, atts, metas = punch_batch(n, m, seed)
    buf = np.frombuffer(b"".join(pk) + bytes(16), np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(x) for x in pk])[:-1]]).astype(np.uint64)
    ln = np.array([len(x) for x in pk], np.uint32)
    mt = realm.PunchMatcher(metas)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(gpu)  # noqa: E731
    match = torch.full((n,), -7, dtype=torch.int32, device=gpu)
    ty = torch.zeros(n, dtype=torch.uint8, device=gpu)
    pad = torch.zeros(n, dtype=torch.int32, device=gpu)
    mt.match_batch(d(buf), d(off), d(ln), n, match, ty, pad, attempts=d(mt.attempts))
    torch.cuda.synchronize()
    hm, ht, hp = match.cpu().numpy(), ty.cpu().numpy(), pad.cpu().numpy()
    hits = 0
    for i, x in enumerate(pk):
        j, t, pd = rref.match(x, atts)
        assert (int(hm[i]), int(ht[i]), int(hp[i])) == (j, t, pd), i   # a miss reports type 0 and padding 0
        hits += j >= 0
    assert n == 1 or 0 < hits < n


# ---------------------------------------------------------------- the edge lattice (tests/wire_cases.py)
GUARD = 64   # sentinel bytes on either side of every output array


def _guarded(nbytes, gpu):
    import torch
    t = torch.full((GUARD + nbytes + GUARD,), wc.SENTINEL, dtype=torch.uint8, device=gpu)
    return t, t[GUARD:GUARD + nbytes]


def _guards_intact(t, nbytes):
    h = t.cpu().numpy()
    return bool((h[:GUARD] == wc.SENTINEL).all() and (h[GUARD + nbytes:] == wc.SENTINEL).all())


def _match_lattice(gpu, n, m, null_out=False, stream=None):
    """The first n lattice entries against the first m attempts; (match, type, padding)
    as numpy arrays, type and padding None when they were passed as null.  The input
    buffer has exactly the lattice's size; 64 guard bytes around each output."""
    import torch
    from hysteria_amd import realm
    lat = wc.punch_lattice()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(gpu)  # noqa: E731
    mt = realm.PunchMatcher([realm.PunchMetadata(nonce.hex(), key.hex()) for nonce, key in lat["attempts"][:m]])
    assert mt.attempts.tobytes() == wc.attempts_bytes(lat["attempts"][:m])
    inp, off = d(lat["buf"]), lat["off"]
    gm, match = _guarded(4 * n, gpu)
    gt, ty = _guarded(n, gpu)
    gp, pad = _guarded(4 * n, gpu)
    torch.cuda.synchronize()
    mt.match_batch(inp, d(off[:n].copy()), d(lat["len"][:n].copy()), n, match, None if null_out else ty,
                   None if null_out else pad, attempts=d(mt.attempts) if m else None, stream=stream)
    (stream.synchronize if stream is not None else torch.cuda.synchronize)()
    assert _guards_intact(gm, 4 * n) and _guards_intact(gt, n) and _guards_intact(gp, 4 * n)
    hm, ht, hp = match.cpu().numpy().view(np.int32), ty.cpu().numpy(), pad.cpu().numpy().view(np.uint32)
    if null_out:   # untouched
        assert (ht == wc.SENTINEL).all() and (pad.cpu().numpy() == wc.SENTINEL).all()
        return hm, None, None
    return hm, ht, hp


def _check_lattice(got, n, m):
    hm, ht, hp = got
    lat = wc.punch_lattice()
    for i, (j, t, pd) in enumerate(wc.punch_expected(n, m)):
        assert int(hm[i]) == j, (i, lat["labels"][i])
        if ht is not None:
            assert (int(ht[i]), int(hp[i])) == (t, pd), (i, lat["labels"][i])


@pytest.mark.parametrize("name,n,m,null_out", wc.punch_runs(), ids=[r[0] for r in wc.punch_runs()])
def test_match_lattice(gpu, name, n, m, null_out):
    """The attempt walk (shared keys, shared nonces, a duplicate attempt: the lowest
    index wins), corrupted padding, unknown types, every single-bit flip of the 33
    deciding bytes, lengths around both limits with no bytes behind the out-of-range
    ones, unsorted and aliased in_off.  match, type and padding of every entry:
    type 0 and padding 0 on a miss."""
    _check_lattice(_match_lattice(gpu, n, m, null_out), n, m)


def test_match_lattice_on_a_side_stream(gpu):
    import torch
    n = len(wc.punch_lattice()["len"])
    _check_lattice(_match_lattice(gpu, n, 5, stream=torch.cuda.Stream(device=gpu)), n, 5)


def test_match_empty_batch_writes_nothing(gpu):
    """n == 0: no launch, the outputs keep their bytes."""
    import torch
    from hysteria_amd import realm
    lat = wc.punch_lattice()
    mt = realm.PunchMatcher([realm.PunchMetadata(nonce.hex(), key.hex()) for nonce, key in lat["attempts"]])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(gpu)  # noqa: E731
    outs = [torch.full((256,), wc.SENTINEL, dtype=torch.uint8, device=gpu) for _ in range(3)]
    mt.match_batch(d(lat["buf"]), d(lat["off"]), d(lat["len"]), 0, *outs, attempts=d(mt.attempts))
    torch.cuda.synchronize()
    assert all(bool((o == wc.SENTINEL).all()) for o in outs)
