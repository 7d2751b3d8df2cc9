"""GPU tier of the Salamander batch kernels' limits lattice (tests/batch_limit_cases.py):
the records the CPU tier runs through the emulated kernels, here through the Python
bindings on the gfx950 kernels.  Per case and kernel setting: the kernel
hyobfs_salamander_batch_kernel reports, the call's status, the whole of `out` with 64
sentinel bytes on either side, out_off, out_len and out_total.  The input tensor ends at
the last byte the header promises; a datagram over the limit points at that end."""
import numpy as np
import pytest

import batch_limit_cases as bl

pytestmark = pytest.mark.gpu

M = bl.M
GUARD = 64


def _unset(width):
    return int.from_bytes(bytes([bl.UNSET]) * width, "little", signed=True)


def _run_case(gpu, cs):
    import torch
    import hysteria_amd
    from hysteria_amd._lib import HyobfsError
    n, cap = cs["n"], cs["out_cap"]
    raw = torch.empty(len(cs["inp"]) + cs["in_align"], dtype=torch.uint8, device=gpu)
    assert raw.data_ptr() % 16 == 0
    inp = raw[cs["in_align"]:]
    inp.copy_(torch.from_numpy(cs["inp"]))
    kw = dict(in_stride=cs["in_stride"], len_uniform=cs["len_uniform"], pkt_cap=cs["pkt_cap"], out_cap=cap,
              out_stride=cs["out_stride"])
    if cs["in_off"] is not None:
        kw["in_off"] = torch.from_numpy(cs["in_off"].view(np.int64)).to(gpu)
    if cs["in_len"] is not None:
        kw["in_len"] = torch.from_numpy(cs["in_len"].view(np.int32)).to(gpu)
    if cs["obf"]:
        kw["salts"] = torch.from_numpy(cs["salts"].view(np.int64)).to(gpu)
    exp = torch.from_numpy(bl.expected_out(cs)).to(gpu)
    exp_off = torch.from_numpy(cs["out_off"].view(np.int64)).to(gpu)
    exp_len = torch.from_numpy(cs["out_len"].view(np.int32)).to(gpu)
    with hysteria_amd.SalamanderObfuscator(cs["psk"], 0) as o:
        for setting, want in cs["settings"]:
            o.set_kernel(setting)
            buf = torch.full((cap + 2 * GUARD,), bl.SENTINEL, dtype=torch.uint8, device=gpu)
            out = buf[GUARD:GUARD + cap]
            assert out.data_ptr() % 16 == 0
            out_off = torch.full((n,), _unset(8), dtype=torch.int64, device=gpu)
            out_len = torch.full((n,), _unset(4), dtype=torch.int32, device=gpu)
            total = torch.full((1,), _unset(8), dtype=torch.int64, device=gpu)
            args = dict(kw, out=out, out_off=out_off, out_len=out_len, out_total=total)
            need = hysteria_amd.SalamanderObfuscator.workspace_bytes(inp=inp, n=n, **{k: v for k, v in args.items()
                                                                                      if k != "salts"})
            ws = torch.full((need + 2 * GUARD,), bl.SENTINEL, dtype=torch.uint8, device=gpu)   # 256-aligned + 64
            if need:
                args.update(workspace=ws[GUARD:GUARD + need], workspace_bytes=need)
            tag = (cs["name"], setting)
            if want == bl.INVALID:
                with pytest.raises(HyobfsError) as e:
                    o.batch_kernel(cs["obf"], inp=inp, n=n, **args)
                assert e.value.status == bl.INVALID, tag
                with pytest.raises(HyobfsError) as e:
                    (o.obfuscate_batch if cs["obf"] else o.deobfuscate_batch)(inp, n, **args)
                assert e.value.status == bl.INVALID, tag
            else:
                assert o.batch_kernel(cs["obf"], inp=inp, n=n, **args) == want, tag
                (o.obfuscate_batch if cs["obf"] else o.deobfuscate_batch)(inp, n, **args)
            torch.cuda.synchronize()
            assert torch.equal(out, exp), (tag, "out", int((out != exp).nonzero()[0]))
            assert bool((buf[:GUARD] == bl.SENTINEL).all()) and bool((buf[GUARD + cap:] == bl.SENTINEL).all()), tag
            assert bool((ws[:GUARD] == bl.SENTINEL).all()) and bool((ws[GUARD + need:] == bl.SENTINEL).all()), tag
            assert torch.equal(out_off, exp_off), (tag, "out_off")
            assert torch.equal(out_len, exp_len), (tag, "out_len")
            assert int(total[0]) == int(np.array([cs["out_total"]], np.uint64).view(np.int64)[0]), (tag, "out_total")


def _check(gpu, names):
    for name in names:
        _run_case(gpu, bl.build(name))


def _groups(names, size):
    return [names[i:i + size] for i in range(0, len(names), size)]


@pytest.mark.parametrize("S", bl.LOW_SLOTS + [bl.LARGE_LOW_SLOT])
def test_slot_estimate(gpu, S):
    """Slots whose float estimate of a chunk's datagram is one too low (328, 376, 656 and
    1 048 360), under AUTO (the tile kernel: its `r >= S` repair) and forced WAVE."""
    names = [n for n in bl.NAMES["slot_estimate"] if n.startswith("est_S%d_" % S)]
    assert names
    _check(gpu, names)


@pytest.mark.parametrize("names", _groups(bl.NAMES["eligibility"], 8), ids=lambda g: g[0])
def test_eligibility_pairs(gpu, names):
    """Each tile_params / fill_params predicate from both sides: the kernel reported, the
    status (out_stride over the limit: HYOBFS_ERR_INVALID, nothing written), the drops."""
    _check(gpu, names)


@pytest.mark.parametrize("names", _groups(bl.NAMES["input_aliasing"], 8), ids=lambda g: g[0])
def test_input_aliasing(gpu, names):
    """Broadcast (in_stride 0), overlapping (in_stride 8), equal and descending offsets."""
    _check(gpu, names)


_UNIFORM = [n for n in bl.NAMES["length_ladder"] if n.startswith("ladder_uniform")]
_REST = [n for n in bl.NAMES["length_ladder"] if n not in _UNIFORM]


@pytest.mark.parametrize("names", _groups(_UNIFORM, 6), ids=lambda g: g[0])
def test_length_ladder_uniform(gpu, names):
    """Uniform slots of 4096 bytes up to M and of every length over it (all dropped)."""
    _check(gpu, names)


@pytest.mark.parametrize("names", _groups(_REST, 2), ids=lambda g: g[0])
def test_length_ladder_ragged_and_contiguous(gpu, names):
    """The ladder among ordinary datagrams: packed output from explicit offsets (AUTO,
    WAVE) and from contiguous input (AUTO, WAVE, FLAT), datagrams at M - 8, M, M + 1 and
    up to 2^32 - 1; offsets after a dropped datagram must not move."""
    _check(gpu, names)


@pytest.mark.parametrize("L", [M, M + 1])
def test_per_packet_calls_at_the_limit(gpu, L):
    """hyobfs_salamander_obfuscate / _deobfuscate on M input bytes (the whole result) and
    on M + 1 (0, nothing written): ties HYOBFS_BATCH_MAX_DATAGRAM to the library."""
    import hysteria_amd
    assert hysteria_amd.BATCH_MAX_DATAGRAM == M
    salt, payload, wire, wire_in, plain = bl.packet_vectors(L)
    with hysteria_amd.SalamanderObfuscator(bl.PSK, 0) as o:
        out = bytearray(b"\xa5" * (L + 8))
        assert o.obfuscate(payload, out, salt=salt) == len(wire)
        assert bytes(out[:len(wire)]) == wire and out[len(wire):] == b"\xa5" * (L + 8 - len(wire))
        back = bytearray(b"\xa5" * L)
        assert o.deobfuscate(wire_in, back) == len(plain)
        assert bytes(back[:len(plain)]) == plain and back[len(plain):] == b"\xa5" * (L - len(plain))
