"""The ACL's geosite regex entries on the GPU (hysteria_amd/csrc/acl.hip, entry kind
kRegex: a lane walks the entry's DFA over the name in LDS) through
RuleSet.match_batch, match_sniffed_batch and match_many, against the restatement
tests/acl_ref.py extended by the regex branch of tests/acl_regex_cases.py (Python's
re under Go's meaning).  The groups are the smallest shapes at which the kernel
can go wrong; tests/test_acl_regex.py runs the same ones under AddressSanitizer."""
import numpy as np
import pytest

import acl_cases as ac
import acl_ref
import acl_regex_cases as rc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64   # sentinel bytes on either side of `res`


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def groups():
    """(group, its rule set on the device) for every group, made once."""
    from hysteria_amd import acl
    out = [(g, acl.RuleSet(ac.product_rules(g[1]))) for g in rc.groups()]
    yield out
    for _, rs in out:
        rs.close()


def _t(dev, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def _res(dev, n):
    buf = torch.full((2 * GUARD + 16 * n,), 0xA5, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + 16 * n]


def _records(buf, n):
    from hysteria_amd import acl
    h = buf.cpu().numpy()
    assert (h[:GUARD] == 0xA5).all() and (h[GUARD + 16 * n:] == 0xA5).all(), "write outside res"
    return np.frombuffer(h[GUARD:GUARD + 16 * n].tobytes(), acl.ACL_RESULT_DTYPE)


def _same(label, items, got, exp):
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        g = (int(g["status"]), int(g["rule"]), int(g["outbound"]), int(g["hijack"]))
        assert g == e, (label, i, items[i], g, e)


def test_groups_cover_the_issue_list(groups):
    labels = {g[0] for g, _ in groups}
    assert labels >= {"rx_items_1", "rx_items_3", "rx_items_4", "rx_items_5", "rx_items_1029", "rx_straddle", "rx_130",
                      "rx_order", "rx_gating", "rx_cn", "rx_lengths", "rx_normalise", "rx_host", "rx_big", "rx_pinned"}
    for g, rs in groups:
        assert rs.flags() == 1, g[0]


def test_match_batch(dev, groups):
    """Every group through RuleSet.match_batch; nothing written outside res."""
    for group, rs in groups:
        label, rules, items = group
        names, off, lens, v4, v6, fl, proto, port = (_t(dev, a) for a in ac.arrays(items))
        buf, res = _res(dev, len(items))
        rs.match_batch(names, off, lens, v4, v6, fl, proto, port, len(items), res, device=0)
        _same(label, items, _records(buf, len(items)), rc.expected(group))


def test_match_sniffed_batch(dev, groups):
    """Every group through RuleSet.match_sniffed_batch: names in rows of a stride
    with sentinel bytes after them, every 7th item a failed sniff and every empty
    name NO_NAME."""
    from hysteria_amd import sniff
    stride = ac.SNIFFED_STRIDE
    seen = set()
    for k, (group, rs) in enumerate(groups):
        label, rules, items = group
        n = len(items)
        st = ac.sniff_statuses(items, k)
        rows = np.full((n, stride), 0xA5, np.uint8)
        sres = np.zeros(n, sniff.SNIFF_RESULT_DTYPE)
        for i, it in enumerate(items):
            if st[i] == 0:
                rows[i, :len(it[0])] = np.frombuffer(it[0], np.uint8)
            sres[i] = (st[i], len(it[0]), 7, 0)
        _, _, _, v4, v6, fl, proto, port = (_t(dev, a) for a in ac.arrays(items))
        buf, res = _res(dev, n)
        rs.match_sniffed_batch(_t(dev, rows.reshape(-1)), stride, _t(dev, sres.view(np.uint8)), v4, v6, fl, proto, port, n,
                               res, device=0)
        exp = rc.expected(group, True, k)
        _same(label, items, _records(buf, n), exp)
        seen |= {e[0] for e in exp}
    assert seen == {0, acl_ref.NO_NAME, acl_ref.HOST}


def test_match_many(dev, groups):
    """Every group through RuleSet.match_many: the names the device leaves to the
    host are finished by the host matcher's regex branch."""
    for group, rs in groups:
        label, rules, items = group
        got = rs.match_many([it[:3] for it in items], [it[3] for it in items], [it[4] for it in items])
        for it, g in zip(items, got):
            r = rc.match(rules, it[:3], it[3], it[4])
            assert g == ((rules[r]["outbound"], None) if r >= 0 else (0, None)), (label, it, g, r)


def test_compiled_fixture_lists_end_to_end(dev):
    """Text rules over the fixture's lists, compiled with device_regex=True, through
    match_many: the reference's pinned case (Test_geositeMatcher_Match, "regexp")
    and the attribute filter in front of the regex entries."""
    import hysteria_amd
    from hysteria_amd import acl
    fx = rc.fixture()

    class Geo:
        def geoip(self, code):
            return None

        def geosite(self, name):
            return [("regex", v, a) for n, v, a in fx["entries"] if n == name] + \
                [tuple(e) for e in fx["extra"].get(name, [])] or None

    text = "ads(geosite:google@ads, tcp)\napple(geosite:apple)\ncn(geosite:cn)\nrest(all)"
    with hysteria_amd.compile_rules(hysteria_amd.parse_text_rules(text), {"ads": 1, "apple": 2, "cn": 3, "rest": 4},
                                    Geo(), device_regex=True) as rs:
        assert isinstance(rs, acl.RuleSet)
        hosts = [fx["pinned"]["name"], "ADSERVICE.GOOGLE.CO.UK.", "adservice.google.co.uk", "x.ap-beijing.myqcloud.com",
                 "cdn5.apple-mapkit.com", "xn--cdn4.apple-mapkit.com", ""]
        got = rs.match_many([(h, None, None) for h in hosts], [1, 1, 2, 1, 1, 1, 1], [443] * 7)
        assert [g[0] for g in got] == [2, 1, 4, 3, 4, 4, 4]
