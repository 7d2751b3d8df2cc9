"""Device rates of Gecko's receive side on the frames that
scripts/aux_bench.py encodes for its Gecko row (same generator, same count: 262144
long-header messages of 1200 B, ~1.3M frames in the default 512..1200 band):

* the new path: hyobfs_gecko_peek_batch over the wire, then hyobfs_gecko_open_batch of
  every message (all complete; the chunk lists are built once on the host, outside
  the timed region);
* today's calls on the same wire: hyobfs_salamander_deobfuscate_batch into packed
  output, then hyobfs_gecko_parse_batch.  That path assembles nothing: it does
  strictly less.

Per call: ms (HIP events around one call, the median of 20 after 3 untimed ones),
datagrams/s and the bytes the call must move (what it has to read and write by its
definition, not what the caches fetch) against 8 TB/s.  Prints one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hysteria_amd  # noqa: E402
from hysteria_amd import gecko  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, warmup=3, rounds=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(dev)


def row(ms, n, nbytes):
    return {"ms": round(ms, 4), "datagrams_per_s": round(n / ms * 1e3), "bytes_moved": int(nbytes),
            "GBs": round(nbytes / ms / 1e6, 1), "frac_of_8TBs": round(nbytes / ms / 1e6 / 8000, 4)}


# ---- the frames of aux_bench.py's Gecko row
M, L = 262144, 1200
rng = np.random.default_rng(1)
fr, off, total = gecko.plan_fragments(np.full(M, L), rand32=lambda k: rng.integers(0, 2**32, k, dtype=np.uint64))
nf = len(fr)
msg = torch.empty(M * L, dtype=torch.uint8, device=dev)
hysteria_amd.synth_stream(msg, M * L, 1, 0)
salts = torch.empty(nf, dtype=torch.int64, device=dev)
hysteria_amd.synth_u64(salts, nf, 2, 0)
wire = torch.empty(total + 16, dtype=torch.uint8, device=dev)
o = hysteria_amd.SalamanderObfuscator(b"average_password", 0)
doff = d(off)
gecko.encode_batch(o, msg=msg, frames=d(fr), salts=salts, pad_key=bytes(range(1, 33)), pad_nonce=bytes(12), out=wire,
                   out_off=doff, n=nf)
wl = d((13 + fr["chunk_len"].astype(np.uint32) + fr["pad_len"]).astype(np.uint32))

# ---- the plan, once, on the host: message j is its frames in order
counts = np.bincount(np.cumsum((fr["idx_total"] >> 4) == 0) - 1, minlength=M)
msg_first = np.zeros(M + 1, np.uint64)
np.cumsum(counts, out=msg_first[1:])
chunk_idx, d_first = d(np.arange(nf, dtype=np.uint32)), d(msg_first)
out_off, out_cap = d(np.arange(M, dtype=np.uint64) * np.uint64(L)), d(np.full(M, L, np.uint32))
parsed = torch.empty(nf * 16, dtype=torch.uint8, device=dev)
keys = torch.empty(nf * 32, dtype=torch.uint8, device=dev)
opened = torch.empty(M * L + 16, dtype=torch.uint8, device=dev)
out_len = torch.empty(M, dtype=torch.int32, device=dev)
status = torch.empty(M, dtype=torch.int32, device=dev)

res = {"messages": M, "msg_len": L, "datagrams": nf, "wire_bytes": total}
ms_peek = timed(lambda: gecko.peek_batch(o, wire, doff, wl, nf, parsed, keys))
ms_open = timed(lambda: gecko.open_batch(wire, doff, wl, parsed, keys, nf, chunk_idx, d_first, M, opened, out_off, out_cap,
                                         out_len, status))
ok = bool((status == 0).all()) and bool((out_len == L).all()) and torch.equal(opened[:M * L], msg)
res["peek"] = row(ms_peek, nf, nf * (8 + 4 + 13 + 16 + 32))
res["open"] = row(ms_open, nf, 2 * M * L + nf * (4 + 16 + 4 + 8 + 32) + M * (8 + 8 + 4 + 4 + 4))
res["peek_plus_open_ms"] = round(ms_peek + ms_open, 4)
res["every_message_opened_exactly"] = ok

# ---- today's calls on the same wire
plain = torch.empty(total + 16, dtype=torch.uint8, device=dev)
poff = torch.empty(nf, dtype=torch.int64, device=dev)
plen = torch.empty(nf, dtype=torch.int32, device=dev)
ws = torch.empty(hysteria_amd.workspace_size(nf), dtype=torch.uint8, device=dev)
ms_deob = timed(lambda: o.deobfuscate_batch(wire, nf, in_off=doff.view(torch.int64), in_len=wl.view(torch.int32), out=plain,
                                            out_cap=total, out_off=poff, out_len=plen, workspace=ws,
                                            workspace_bytes=ws.numel()))
today = torch.empty(nf * 16, dtype=torch.uint8, device=dev)
ms_parse = timed(lambda: gecko.parse_batch(plain, poff, plen, nf, today))
res["deobfuscate"] = row(ms_deob, nf, total + (total - 8 * nf) + nf * (8 + 4 + 8 + 4))
res["parse"] = row(ms_parse, nf, nf * (8 + 4 + 5 + 16))
res["deobfuscate_plus_parse_ms"] = round(ms_deob + ms_parse, 4)
res["peek_records_equal_parse_records"] = torch.equal(parsed, today)
o.close()
print(json.dumps(res))
if not (ok and res["peek_records_equal_parse_records"]):
    sys.exit(1)
