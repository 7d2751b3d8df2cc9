"""GPU tier of the wave kernel's chunk-ownership lattice (tests/wave_chunk_cases.py): the
records the CPU tier runs through the emulated kernels, here through the Python bindings
on the gfx950 kernels, every case under AUTO and WAVE and the contiguous packed copies
under FLAT as well.  Per case and setting (tests/test_gpu_batch_limits.py's _run_case):
the kernel hyobfs_salamander_batch_kernel reports, the whole of `out` with 64 sentinel
bytes on either side, a workspace of exactly workspace_bytes with sentinel bytes around
it, out_off, out_len and out_total."""
import pytest

import wave_chunk_cases as wc
from test_gpu_batch_limits import _run_case

pytestmark = pytest.mark.gpu


def _check(gpu, names):
    for name in names:
        cs = wc.build(name)
        assert dict(cs["settings"])["wave"] == "wave" and dict(cs["settings"])["auto"] == "wave"
        assert ("flat" in dict(cs["settings"])) == wc.contiguous_packed(name)
        _run_case(gpu, cs)


def _groups(names, size):
    return [names[i:i + size] for i in range(0, len(names), size)]


@pytest.mark.parametrize("names", _groups(wc.NAMES["phase_width"], 4), ids=lambda g: g[0])
def test_phase_width(gpu, names):
    """Every (output offset mod 32, width) pair at a group's first, last and an inner
    lane; free-form input of every phase mod 16 and its contiguous copy."""
    _check(gpu, names)


@pytest.mark.parametrize("family", ["neighbours", "crowded", "empty", "slots"])
def test_family(gpu, family):
    """Every triple of neighbouring widths; up to 40 datagrams in three chunks; dropped
    stretches over whole groups and a whole prefix tile; groups that ask for 63, 64, 65
    and more park slots."""
    _check(gpu, wc.NAMES[family])


@pytest.mark.parametrize("after", wc.CUT_AFTER)
def test_out_cap_cuts(gpu, after):
    """out_cap at every byte within 17 of the end of datagram 31, 32 and 63: nothing past
    out_cap is written, no offset moves."""
    _check(gpu, [n for n in wc.NAMES["out_cap"] if "_e%d_" % after in n])


@pytest.mark.parametrize("d", ["obf", "deobf"])
def test_slotted_strides(gpu, d):
    """Slots of 9..1201 bytes that are no chunk multiples, full and ragged: neighbouring
    runs belong to different waves, the sentinel in every gap survives."""
    _check(gpu, [n for n in wc.NAMES["strides"] if n.startswith("stride_%s_" % d)])
