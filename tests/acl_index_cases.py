"""Cases for the hashed index over a DOMAIN_SET's FULL and ROOT values
(include/hyobfs_acl.h, "THE INDEX"), shared by the CPU tier
(tests/test_acl_index.py) and the GPU tier (tests/test_gpu_acl_index.py).  TEST
INFRASTRUCTURE ONLY.

Case groups are tests/acl_cases.py's (label, rules, items).  What a group must
give comes from the restatement alone: tests/acl_regex_cases.py's ``expected``
(tests/acl_ref.py with the regex branch), imported and not edited.  Every group
is compiled with HYOBFS_ACL_FLAG_REGEX | HYOBFS_ACL_FLAG_INDEX and the
``index_min`` of INDEX_MIN (1 where it says nothing), and again without the
index; the two must give the same records.
"""
import random

import acl_cases as ac
import acl_regex_cases as rc

R, item, number = ac.R, ac.item, ac.number
FLAG_REGEX, FLAG_INDEX = 1, 2
INDEX_MIN = {"ix_threshold_3": 3, "ix_threshold_65": 0}   # 0: the library's default, 65
# (entries of the walk table, {rule: (values, slots)} of the rules that have an index) where a group pins them
SHAPE = {}


def index_min(label):
    return INDEX_MIN.get(label, 1)


def dset(*entries, **kw):
    return R("domain_set", entries=list(entries), **kw)


def _labels_name(last, first=b"a"):
    """255 bytes: 128 one-byte labels."""
    labs = [first] + [bytes([97 + k % 26]) for k in range(1, 127)] + [last]
    name = b".".join(labs)
    assert len(name) == 255
    return name


def seeded_values(n, seed, labels=(2, 2, 2, 3)):
    """n distinct lower-case names of mostly two labels."""
    rnd = random.Random(seed)
    out = set()
    while len(out) < n:
        labs = ["".join(rnd.choice("abcdefghijklmnopqrstuvwxyz0123456789-") for _ in range(rnd.randrange(1, 12)))
                for _ in range(rnd.choice(labels) - 1)]
        out.add(".".join(labs + [rnd.choice(("com", "cn", "net", "org", "io"))]).encode())
    return sorted(out)


def groups():
    out = []
    # item counts round the four-wave workgroup
    rules = number([dset(("root", b"mimi.test"), ("full", b"exact.test"), ("root", b"b.c")),
                    dset(("root", b"test"), ("plain", b"keyword"))])
    pool = [b"mimi.test", b"x.mimi.test", b"xmimi.tes", b"exact.test", b"x.exact.test", b"a.b.c", b"ab.c", b"",
            b"none.org", b"a-keyword.org", b"MIMI.TEST."]
    for n in (1, 3, 4, 5, 1029):
        out.append(("ix_items_%d" % n, rules, [item(pool[(7 * i) % len(pool)]) for i in range(n)]))
    SHAPE["ix_items_1"] = (3, {0: (3, 8), 1: (1, 2)})

    # the rule at its edges
    rules = number([dset(("root", b".b")), dset(("root", b"b")), dset(("full", b"value")), dset(("root", b"value")),
                    dset(("full", b"onlyfull.test")),
                    dset(("full", b"both.test"), ("root", b"both.test"), ("root", b"twice.test"), ("root", b"twice.test"))])
    names = [b"value", b"x.value", b"xvalue", b"value.x", b".value", b"a..b", b"a.b", b".b", b"b", b"ab", b"..b",
             b"onlyfull.test", b"x.onlyfull.test", b"both.test", b"x.both.test", b"twice.test", b"y.twice.test",
             b"ytwice.test", b"x.y.value", b"value.", b"VALUE", b"", b"."]
    out.append(("ix_boundary", rules, [item(x) for x in names]))
    SHAPE["ix_boundary"] = (6, {0: (1, 2), 1: (1, 2), 2: (1, 2), 3: (1, 2), 4: (1, 2), 5: (2, 4)})

    # the empty value, as ROOT and as FULL, each alone in a set
    rules = number([dset(("root", b""), proto=1), dset(("full", b""))])
    out.append(("ix_empty", rules, [item(x, proto=p) for x in (b"", b"....", b"a", b"a.", b".a", b".") for p in (1, 2)]))

    # 128 candidates; the LDS rounds; value lengths round the 16 inline bytes of a linear entry
    whole, last, miss = _labels_name(b"q"), _labels_name(b"7", b"b"), _labels_name(b"0", b"c")
    lens = (63, 64, 65, 128, 129, 192, 193, 255)
    byl = {n: ac._name_of(n, n) for n in lens}
    vals = {n: (b"0123456789abcdefgh"[:n - 5] + b".test")[-n:] for n in (15, 16, 17)}
    long_value = ac._name_of(255, 5)
    rules = number([dset(("full", whole), ("root", b"7")),
                    dset(*[("full", byl[n]) for n in lens]),
                    dset(*[("root", byl[n][9:]) for n in lens if n > 64]),
                    dset(("root", b"z"), *[("root", v) for v in vals.values()], ("root", long_value))])
    names = [whole, last, miss, whole[2:], b"x" + whole[1:]]
    for n in lens:
        names += [byl[n], bytes([byl[n][0] ^ 1]) + byl[n][1:], byl[n][:-1] + bytes([byl[n][-1] ^ 1])]
        if n > 64:
            names += [b"q." + byl[n][9:], b"q" + byl[n][9:]]
    for v in list(vals.values()) + [b"z"]:
        names += [v, b"x." + v, b"x" + v, b"Z" + v[1:], b"x.Z" + v[1:]]
    names += [long_value, long_value[:-1] + b"0", b"y" + long_value[1:]]
    out.append(("ix_labels", rules, [item(x) for x in names]))

    # the threshold: PLAIN and REGEX entries do not count
    for label, m in (("ix_threshold_3", 3), ("ix_threshold_65", 65)):
        def ents(k):
            return [("root" if i % 3 else "full", b"v%d.thr.test" % i) for i in range(k)] + \
                [("plain", b"plainthr"), ("regex", b"^rx[0-9]+\\.thr\\.test$")]
        rules = number([dset(*ents(m - 1)), dset(*ents(m), ("plain", b"second")), R("suffix", pattern=b"thr.test")])
        names = [b"v0.thr.test", b"x.v0.thr.test", b"x.v1.thr.test", b"v%d.thr.test" % (m - 2), b"v%d.thr.test" % (m - 1),
                 b"x.v%d.thr.test" % (m - 1), b"v%d.thr.test" % m, b"a-plainthr.org", b"the-second.org", b"rx77.thr.test",
                 b"rx.thr.test", b"none.org"]
        out.append((label, rules, [item(x) for x in names]))
        slots = 2
        while slots < 2 * m:
            slots *= 2
        SHAPE[label] = ((m - 1 + 2) + (1 + 3) + 1, {1: (m, slots)})

    # indexed values, PLAIN and REGEX entries in one set; order; gating
    rules = number([R("suffix", pattern=b"early.test"),
                    dset(("root", b"idx.test"), ("full", b"f.idx.test"), ("root", b"early.test"), ("plain", b"plainword"),
                         ("regex", b"^rx[0-9]+\\.test$")),
                    dset(("root", b"idx.test"), ("root", b"second.test")),
                    dset(("root", b"gated.test"), proto=1, ports=(80, 90)),
                    dset(("root", b"gated.test"), ("root", b"idx.test"))])
    items = [item(x) for x in (b"a.idx.test", b"f.idx.test", b"x.f.idx.test", b"x.early.test", b"has-plainword.org",
                               b"rx12.test", b"rx.test", b"a.second.test", b"none.org")]
    items += [item(b"gated.test", proto=p, port=q) for p in (1, 2) for q in (79, 80, 85, 90, 91, 443)]
    out.append(("ix_mixed", rules, items))
    SHAPE["ix_mixed"] = (1 + 3 + 1 + 1 + 1, {1: (3, 8), 2: (2, 4), 3: (1, 2), 4: (2, 4)})

    # the index entry at table positions 62 to 65
    for n in (62, 63, 64, 65):
        rules = number([R("exact", pattern=b"p%d.test" % k) for k in range(n)]
                       + [dset(("root", b"in.set"), ("full", b"full.set"), ("plain", b"plainset")), R("suffix", pattern=b"set")])
        names = [b"p0.test", b"p%d.test" % (n - 1), b"p%d.test" % n, b"x.in.set", b"full.set", b"x.full.set",
                 b"a-plainset.org", b"other.set", b"none.org"]
        out.append(("ix_straddle_%d" % n, rules, [item(x) for x in names]))
        SHAPE["ix_straddle_%d" % n] = (n + 3, {n: (2, 4)})

    # values that match no name the device decides; names left to the host; normalisation in front of the index
    rules = number([dset(("root", b"Upper.test"), ("full", b"UPPER.TEST"), ("root", b"caf\xc3\xa9.fr"),
                         ("root", b"xn--abc.com"), ("root", b"dot.test."), ("full", b"dot.test.")),
                    dset(("root", b"ok.test"), ("full", b"full.ok"))])
    names = [b"upper.test", b"UPPER.TEST", b"Upper.test", b"x.upper.test", b"dot.test", b"dot.test.", b"dot.test..",
             b"x.dot.test.", b"xn--abc.com", b"a.xn--abc.com", b"caf\xc3\xa9.fr", b"a\x80.ok.test", b"OK.TEST", b"a.ok.test..",
             b"Full.OK.", b"x.full.ok", b"A.XN--b.ok.test"]
    out.append(("ix_never", rules, [item(x) for x in names]))

    # natural chains at load <= 0.5
    vals = seeded_values(5200, 77)
    roots, fulls = vals[:5000], vals[5000:]
    rules = number([dset(*[("root", v) for v in roots], *[("full", v) for v in fulls]), R("all")])
    names = []
    for v in vals[::50]:
        names += [v, b"www." + v]
    names += [b"miss%d." % k + vals[(31 * k) % 5200].rsplit(b".", 1)[0] + b".example" for k in range(200)]
    out.append(("ix_big", rules, [item(x) for x in names]))
    SHAPE["ix_big"] = (2, {0: (5200, 16384)})

    # cn's 200 roots and 37 regexes of the fixture
    cn = [g for g in rc.groups() if g[0] == "rx_cn"][0]
    out.append(("ix_cn", cn[1], cn[2]))
    SHAPE["ix_cn"] = (1 + 37 + 1, {0: (200, 512)})
    return out


def weak_groups():
    """What the weak-hash binary runs beside ix_boundary and ix_mixed: 40 values,
    every probe sequence begins in one of four slots of 128."""
    vals = seeded_values(40, 5)
    rules = number([dset(*[("root" if k % 4 else "full", v) for k, v in enumerate(vals)])])
    names = []
    for v in vals:
        names += [v, b"x." + v, b"x" + v]
    return [("ix_weak_40", rules, [item(x) for x in names] + [item(b"none.org"), item(b"")])]


def property_group(sets=300, n_names=2000, seed=3):
    """Seeded sets of 1-12 FULL / ROOT values and seeded names, both over {a, b, .} up
    to 8 bytes.  Set k is rule k of one rule set and takes port k + 1 only, and name
    i comes with port i % sets + 1: every name is matched against exactly one set."""
    rnd = random.Random(seed)

    def text():
        return bytes(rnd.choice(b"ab.") for _ in range(rnd.randrange(0, 9)))
    rules = number([dset(*[(rnd.choice(("root", "full")), text()) for _ in range(rnd.randrange(1, 13))], ports=(k + 1, k + 1))
                    for k in range(sets)])
    return ("ix_property", rules, [item(text(), port=i % sets + 1) for i in range(n_names)])
