"""Cost of geosite regex entries in the batched ACL matcher (hysteria_amd/csrc/acl.hip,
entry kind kRegex: a lane walks the entry's DFA over the name), one GPU, one process,
every timing the median of per-step HIP event times after warm-up (as bench_acl.py):

  base       bench_acl.py's 64-rule set (two DOMAIN_SETs of 4096 root entries, one
             CIDR_SET of 8192) without regexes; a build without regex support runs
             this leg alone, so that it can be compared across commits
  cn         the same set, rule 20's DOMAIN_SET carrying the 37 regexes of the
             geosite database's list `cn` (tests/golden/geosite_regex.json)
  not_cn     the same with the 106 regexes of `geolocation-!cn`

each over N names in three mixes: `mixed` (a third each matching an early rule, a
late rule and none, bench_acl.py's), `early` (every name decided before the regex
entries are reached) and `miss` (every name walks every entry, the regex steps
included), and for the regex sets `regex_hit` (names that a regex entry matches).
The regex entries stand after their rule's 4096 other entries, so the 37 are one
more 64-entry step and the 106 two; `extra_us_per_step_and_wave` is the added time
of the miss mix per added step, for one of the 7168 resident waves.

Prints one JSON line.

  python scripts/bench_acl_regex.py [--n 262144] [--steps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

RESIDENT_WAVES = 256 * 4 * 7   # 7 waves per SIMD for acl_kernel<0>
SET_RULE = 20                  # the DOMAIN_SET that gets the regex entries


def regex_lists():
    with open(os.path.join(ROOT, "tests", "golden", "geosite_regex.json"), encoding="utf-8") as f:
        fx = json.load(f)
    return {name: [(v, fx["samples"][v]) for n, v, a in fx["entries"] if n == name] for name in ("cn", "geolocation-!cn")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    from bench_acl import names_for, rule_set
    from hysteria_amd import acl, sniff
    dev = torch.device("cuda", 0)
    n = args.n
    rng = np.random.default_rng(7)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    have_regex = hasattr(acl, "regex_check")

    d_res = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    d_v4 = torch.from_numpy(np.tile(np.array([192, 0, 2, 1], np.uint8), n)).to(dev)
    d_v6 = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_fl = torch.ones(n, dtype=torch.uint8, device=dev)
    d_proto = torch.full((n,), acl.PROTO_TCP, dtype=torch.uint8, device=dev)
    d_port = torch.full((n,), 443, dtype=torch.int16, device=dev)

    def leg(rs, temps):
        """Median ms of match_batch over n names drawn from `temps` [(name, rule it must hit)]."""
        pick = rng.integers(0, len(temps), n)
        lens = np.array([len(t[0]) for t in temps], np.uint32)[pick]
        off = np.zeros(n, np.uint64)
        np.cumsum(lens[:-1], out=off[1:])
        blob = np.frombuffer("".join(temps[i][0] for i in pick).encode() + bytes(16), np.uint8).copy()
        want = np.array([t[1] for t in temps], np.int32)[pick]
        d_names, d_off, d_len = (torch.from_numpy(a).to(dev) for a in (blob, off, lens))
        ms = []
        for step in range(args.warmup + args.steps):
            ev[0].record()
            rs.match_batch(d_names, d_off, d_len, d_v4, d_v6, d_fl, d_proto, d_port, n, d_res)
            ev[1].record()
            torch.cuda.synchronize()
            if step >= args.warmup:
                ms.append(ev[0].elapsed_time(ev[1]))
        res = np.frombuffer(d_res.cpu().numpy().tobytes(), acl.ACL_RESULT_DTYPE)
        assert (res["status"] == 0).all() and (res["rule"] == want).all(), np.unique(res["status"])
        med = float(np.median(ms))
        return {"ms": round(med, 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)], "names_per_s": round(n / (med / 1e3))}

    line = {"metric": "ACL match_batch with geosite regex entries, ms per batch of n_names", "unit": "ms", "n_names": n,
            "steps": args.steps, "sets": {}}
    lists = regex_lists() if have_regex else {}
    for label, regexes in [("base", [])] + [(k.replace("geolocation-!cn", "not_cn"), v) for k, v in lists.items()]:
        rs = rule_set(64, True)
        rs.rules[SET_RULE].entries += [("regex", v) for v, _ in regexes]
        mixes = {"mixed": names_for(rs, "mixed"), "early": names_for(rs, "early"), "miss": names_for(rs, "none")}
        if regexes:
            mixes["regex_hit"] = [(s, SET_RULE) for _, s in regexes]
        out = {"regex_entries": len(regexes), "regex_steps": (len(regexes) + 63) // 64}
        for mix, temps in mixes.items():
            out[mix] = leg(rs, temps)
        line["sets"][label] = out
        rs.close()
    base = line["sets"]["base"]
    for label, out in line["sets"].items():
        if out["regex_steps"]:
            for mix in ("mixed", "early", "miss"):
                out[mix]["added_ms"] = round(out[mix]["ms"] - base[mix]["ms"], 4)
            out["extra_us_per_step_and_wave"] = round(out["miss"]["added_ms"] * 1e3 * RESIDENT_WAVES / n / out["regex_steps"], 3)
    line["value"] = base["mixed"]["ms"]
    line["timing"] = "median of per-step HIP event times after warm-up, one process"
    line["build_id"] = sniff._slib().hyobfs_build_id().decode()
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
