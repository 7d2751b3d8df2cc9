"""Cost of the batched ACL matcher (hysteria_amd/csrc/acl.hip) on one GPU, three legs
in one process, every timing the median of per-step HIP event times after warm-up:

  sets    hyobfs_acl_match_batch over N names (a third each matching an early rule,
          a late rule and no rule) against three rule sets: 16 rules, 256 rules,
          and 64 rules of which two are DOMAIN_SETs of 4096 entries and one a
          CIDR_SET of 8192
  fused   hyobfs_quic_sniff_batch, then hyobfs_acl_match_sniffed_batch on the same
          stream (the 256-rule set), against hyobfs_quic_sniff_batch alone, the
          two interleaved step by step over bench_sniff.py's client Initials
  where   the 256-rule set again, all N names matching early / late / nothing

Prints one JSON line (ms per batch and names/s everywhere).

  python scripts/bench_acl.py [--n 262144] [--steps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def rule_set(n_rules, big_sets=False):
    """n_rules rules over all kinds; with big_sets rules 20 and 40 are DOMAIN_SETs of
    4096 root entries and rule 50 a CIDR_SET of 8192 /24s.  No rule matches
    *.example.net or 192.0.2.0/24 but the last, a suffix rule for example.net that
    is UDP only (the fused leg's packets match it, the TCP names do not)."""
    from hysteria_amd import acl
    rules = []
    for i in range(n_rules):
        if big_sets and i in (20, 40):
            r = acl.Rule(acl.KIND_DOMAIN_SET, entries=[("root", "d%d.set%d.test" % (k, i)) for k in range(4096)])
        elif big_sets and i == 50:
            r = acl.Rule(acl.KIND_CIDR_SET, entries=[(bytes([10 + (k >> 12), (k >> 4) & 0xFF, (k & 15) << 4, 0]), 24)
                                                     for k in range(8192)])
        elif i == n_rules - 1:
            r = acl.Rule(acl.KIND_DOMAIN_SUFFIX, pattern="example.net")
            r.proto = acl.PROTO_UDP
        elif i % 16 == 5:
            r = acl.Rule(acl.KIND_CIDR, ip=bytes([172, 16 + i % 16, i & 0xFF, 0]), prefix=24)
        elif i % 8 == 3:
            r = acl.Rule(acl.KIND_DOMAIN_WILDCARD, pattern="*.w%d.zone%d.test" % (i, i % 7))
        elif i % 8 == 6:
            r = acl.Rule(acl.KIND_DOMAIN_EXACT, pattern="www.r%d.zone%d.test" % (i, i % 7))
        else:
            r = acl.Rule(acl.KIND_DOMAIN_SUFFIX, pattern="r%d.zone%d.test" % (i, i % 7))
        r.outbound, r.line_num = 1 + i % 5, i + 1
        rules.append(r)
    return acl.RuleSet(rules)


def name_for(rs, i, k):
    """A name that rule i of rs matches first (i is a domain rule)."""
    from hysteria_amd import acl
    r = rs.rules[i]
    if r.kind == acl.KIND_DOMAIN_SET:
        return "h%d.%s" % (k, r.entries[(k * 7) % len(r.entries)][1])
    p = r.pattern
    return p.replace("*", "h%d" % k) if r.kind == acl.KIND_DOMAIN_WILDCARD else p if r.kind == acl.KIND_DOMAIN_EXACT \
        else "h%d.%s" % (k, p)


def names_for(rs, where, count=4096):
    """`count` template names and the rule each must hit (-1: none): early = one of
    the first four domain rules, late = one of the last four before the final one."""
    from hysteria_amd import acl
    dom = [i for i, r in enumerate(rs.rules[:-1]) if r.kind in (acl.KIND_DOMAIN_EXACT, acl.KIND_DOMAIN_WILDCARD,
                                                                 acl.KIND_DOMAIN_SUFFIX, acl.KIND_DOMAIN_SET)]
    out = []
    for k in range(count):
        w = where if where != "mixed" else ("early", "late", "none")[k % 3]
        if w == "none":
            out.append(("host%04d.sub%d.example.net" % (k, k % 5), -1))
        else:
            i = dom[(k // 3) % 4] if w == "early" else dom[-1 - (k // 3) % 4]
            out.append((name_for(rs, i, k), i))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    from bench_sniff import templates
    from hysteria_amd import acl, quic, sniff
    dev = torch.device("cuda", 0)
    n = args.n
    rng = np.random.default_rng(7)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fns, before=None):
        """Median / min / max ms of each of fns, interleaved step by step."""
        ms = {k: [] for k in fns}
        for step in range(args.warmup + args.steps):
            for k, f in fns.items():
                if before:
                    before()
                ev[0].record()
                f()
                ev[1].record()
                torch.cuda.synchronize()
                if step >= args.warmup:
                    ms[k].append(ev[0].elapsed_time(ev[1]))
        return {k: {"ms": round(float(np.median(v)), 4), "ms_min_max": [round(min(v), 4), round(max(v), 4)],
                    "names_per_s": round(n / (float(np.median(v)) / 1e3))} for k, v in ms.items()}

    d_res = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    d_v4 = torch.from_numpy(np.tile(np.array([192, 0, 2, 1], np.uint8), n)).to(dev)
    d_v6 = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_fl = torch.ones(n, dtype=torch.uint8, device=dev)
    d_proto = torch.full((n,), acl.PROTO_TCP, dtype=torch.uint8, device=dev)
    d_port = torch.full((n,), 443, dtype=torch.int16, device=dev)

    def batch(rs, where):
        """The device arrays of n names drawn from names_for(rs, where), and the rule each must hit."""
        temps = names_for(rs, where)
        pick = rng.integers(0, len(temps), n)
        lens = np.array([len(t[0]) for t in temps], np.uint32)[pick]
        off = np.zeros(n, np.uint64)
        np.cumsum(lens[:-1], out=off[1:])
        blob = np.frombuffer("".join(temps[i][0] for i in pick).encode() + bytes(16), np.uint8).copy()
        want = np.array([t[1] for t in temps], np.int32)[pick]
        return torch.from_numpy(blob).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(lens).to(dev), want

    def leg(rs, where):
        d_names, d_off, d_len, want = batch(rs, where)
        t = timed({"match": lambda: rs.match_batch(d_names, d_off, d_len, d_v4, d_v6, d_fl, d_proto, d_port, n, d_res)})
        res = np.frombuffer(d_res.cpu().numpy().tobytes(), acl.ACL_RESULT_DTYPE)
        assert (res["status"] == 0).all() and (res["rule"] == want).all(), (where, np.unique(res["status"]))
        return t["match"]

    sets = {"rules_16": rule_set(16), "rules_256": rule_set(256), "rules_64_two_domain_sets_one_cidr_set": rule_set(64, True)}
    line = {"metric": "ACL match_batch names/s, device resident, 256 rules, a third each early / late / no match",
            "unit": "names/s", "n_names": n, "steps": args.steps, "sets": {}, "where": {}}
    for label, rs in sets.items():
        line["sets"][label] = dict(leg(rs, "mixed"), entries=sum(max(len(r.entries), 1) if r.kind == acl.KIND_DOMAIN_SET
                                                                 else 1 for r in rs.rules))
    line["value"] = line["sets"]["rules_256"]["names_per_s"]
    for where in ("early", "late", "none"):
        line["where"][where] = leg(sets["rules_256"], where)

    # the fused chain over bench_sniff.py's packets
    temps = templates()
    pick = rng.integers(0, len(temps), n)
    lens = np.array([len(temps[i][0]) for i in pick], np.uint32)
    off = np.zeros(n, np.uint64)
    np.cumsum(lens[:-1], out=off[1:])
    src = torch.from_numpy(np.concatenate([np.frombuffer(temps[i][0], np.uint8) for i in pick] +
                                          [np.zeros(64, np.uint8)])).to(dev)
    buf = torch.empty_like(src)
    d_off, d_len = torch.from_numpy(off).to(dev), torch.from_numpy(lens).to(dev)
    cap, stride = 1024, 255
    d_out = torch.empty(n * cap, dtype=torch.uint8, device=dev)
    d_oo = torch.from_numpy(np.arange(n, dtype=np.uint64) * np.uint64(cap)).to(dev)
    d_cap = torch.full((n,), cap, dtype=torch.int32, device=dev)
    d_qres = torch.empty(n * 24, dtype=torch.uint8, device=dev)
    d_names = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    d_sres = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    ws = torch.empty(sniff.quic_sniff_workspace_size(n), dtype=torch.uint8, device=dev)
    d_udp = torch.full((n,), acl.PROTO_UDP, dtype=torch.uint8, device=dev)
    rs = sets["rules_256"]
    rs.device_set(0)

    def sniff_only():
        sniff.quic_sniff_batch(buf, d_off, d_len, n, d_out, d_oo, d_cap, d_qres, d_names, stride, d_sres, ws)

    def sniff_acl():
        sniff_only()
        rs.match_sniffed_batch(d_names, stride, d_sres, d_v4, d_v6, d_fl, d_udp, d_port, n, d_res)

    t = timed({"sniff_acl": sniff_acl, "sniff": sniff_only,
               "acl": lambda: rs.match_sniffed_batch(d_names, stride, d_sres, d_v4, d_v6, d_fl, d_udp, d_port, n, d_res)},
              before=lambda: buf.copy_(src))   # the sniff works in place: restore the packets (not timed)
    res = np.frombuffer(d_res.cpu().numpy().tobytes(), acl.ACL_RESULT_DTYPE)
    assert (res["status"] == 0).all() and (res["rule"] == 255).all(), np.unique(res["rule"])
    line["fused"] = {"sniff_then_acl": t["sniff_acl"], "sniff_alone": t["sniff"], "acl_stage_alone": t["acl"],
                     "added_ms": round(t["sniff_acl"]["ms"] - t["sniff"]["ms"], 4),
                     "added_fraction": round(t["sniff_acl"]["ms"] / t["sniff"]["ms"] - 1, 4),
                     "note": "every packet's name matches the last of 256 rules: the longest walk this set has"}
    line["timing"] = "median of per-step HIP event times after warm-up; legs of one group interleaved in one process"
    line["build_id"] = sniff._slib().hyobfs_build_id().decode()
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
