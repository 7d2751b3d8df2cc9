"""Writes tests/golden/geosite_regex.json from the reference's geosite database.

TEST INFRASTRUCTURE ONLY; runs where the reference tree is at hand:

    python tests/golden/gen_geosite_regex.py <reference>/extras/outbounds/acl/v2geo/geosite.dat

The fixture holds data only:
  "entries"  every regex entry of the database as [list (lower case), value, attributes]
  "samples"  per distinct value one name that matches it, made by walking the
             parsed pattern (and checked here with Python's re)
  "extra"    for the lists the tests compile or mix (cn, apple, google) some of
             their other entries as [type, value, attributes]
  "pinned"   the reference's own case (Test_geositeMatcher_Match, "regexp")
"""
import json
import os
import re
import sys

TYPES = {0: "plain", 1: "regex", 2: "root", 3: "full"}
EXTRA = {"cn": ("root", 200), "apple": ("root", 20), "google": ("root", 20)}


def varint(b, i):
    v = s = 0
    while True:
        c = b[i]
        i += 1
        v |= (c & 0x7F) << s
        s += 7
        if c < 0x80:
            return v, i


def fields(b):
    """(field number, value) of one protobuf message: varints and length-delimited fields."""
    i = 0
    while i < len(b):
        k, i = varint(b, i)
        f, w = k >> 3, k & 7
        if w == 0:
            v, i = varint(b, i)
        elif w == 2:
            n, i = varint(b, i)
            v = b[i:i + n]
            i += n
        elif w in (1, 5):
            n = 8 if w == 1 else 4
            v = b[i:i + n]
            i += n
        else:
            raise ValueError("wire type %d" % w)
        yield f, v


def read_lists(data):
    """GeoSiteList -> {list name (lower case): [(type, value, attributes)]}."""
    out = {}
    for f, site in fields(data):
        if f != 1:
            continue
        code, doms = None, []
        for f2, v2 in fields(site):
            if f2 == 1:
                code = v2.decode()
            elif f2 == 2:
                typ, val, attrs = 0, b"", []
                for f3, v3 in fields(v2):
                    if f3 == 1:
                        typ = v3
                    elif f3 == 2:
                        val = v3
                    elif f3 == 3:
                        attrs += [v4.decode() for f4, v4 in fields(v3) if f4 == 1]
                doms.append((TYPES[typ], val.decode("utf-8"), attrs))
        out[code.lower()] = doms
    return out


# ------------------------------------------------------------------ one matching name per pattern
class Sampler:
    """Walks a pattern of the database's small language (literals, escapes, '.',
    classes, groups, '|', repeats, anchors) and writes down one text it matches:
    the first branch of an alternation, the fewest repeats (one for '+' and '*')."""

    PREFER = "abcdefghijklmnopqrstuvwxyz0123456789-."

    def __init__(self, p):
        self.p, self.i = p, 0

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else None

    def pick(self, ok):
        for c in self.PREFER:
            if ok(c):
                return c
        raise ValueError("no plain character for a class of %r" % self.p)

    def klass(self):
        neg = self.peek() == "^"
        self.i += neg
        members = set()
        while self.peek() != "]":
            c = self.p[self.i]
            self.i += 1
            if c == "\\":
                c = self.p[self.i]
                self.i += 1
                if c == "d":
                    members |= set("0123456789")
                    continue
                assert not c.isalnum(), self.p
            if self.peek() == "-" and self.p[self.i + 1] != "]":
                hi = self.p[self.i + 1]
                self.i += 2
                members |= {chr(x) for x in range(ord(c), ord(hi) + 1)}
            else:
                members.add(c)
        self.i += 1
        return self.pick(lambda c: (c in members) != neg)

    def atom(self):
        c = self.p[self.i]
        self.i += 1
        if c == "(":
            if self.p.startswith("?:", self.i):
                self.i += 2
            s = self.alt()
            assert self.peek() == ")", self.p
            self.i += 1
            return s
        if c == "[":
            return self.klass()
        if c == ".":
            return "x"
        if c in "^$":
            return ""
        if c == "\\":
            c = self.p[self.i]
            self.i += 1
            if c == "d":
                return "7"
            assert not c.isalnum(), self.p
        return c

    def repeat(self):
        s = self.atom()
        c = self.peek()
        n = 1
        if c in ("*", "+", "?"):
            self.i += 1
        elif c == "{":
            m = re.match(r"\{(\d+)(?:,(\d*))?\}", self.p[self.i:])
            self.i += m.end()
            n = max(int(m.group(1)), 1)
        if self.peek() == "?":
            self.i += 1
        return s * n

    def alt(self):
        first = None
        while True:
            s = ""
            while self.peek() not in (None, "|", ")"):
                s += self.repeat()
            first = s if first is None else first
            if self.peek() != "|":
                return first
            self.i += 1


def to_py(p):
    """Go's '^', '$' for Python's re (the database uses no \\s)."""
    out, i, inclass = "", 0, False
    while i < len(p):
        c = p[i]
        if c == "\\":
            out += p[i:i + 2]
            i += 2
            continue
        if inclass:
            inclass = c != "]"
            out += c
        elif c == "[":
            inclass = True
            out += c
        else:
            out += {"^": "\\A", "$": "\\Z"}.get(c, c)
        i += 1
    return out


def main(path):
    lists = read_lists(open(path, "rb").read())
    entries = [[name, v, a] for name, doms in lists.items() for t, v, a in doms if t == "regex"]
    samples = {}
    for value in sorted({e[1] for e in entries}):
        s = Sampler(value)
        name = s.alt()
        assert s.i == len(value), value
        assert name == name.lower().rstrip(".") and re.search(to_py(value), name), (value, name)
        samples[value] = name
    extra = {}
    for name, (typ, count) in EXTRA.items():
        extra[name] = [[t, v, a] for t, v, a in lists[name] if t == typ][:count]
        assert len(extra[name]) == count, name
    pinned = {"list": "apple", "name": "cdn4.apple-mapkit.com", "want": True}
    assert any(re.search(to_py(v), pinned["name"]) for n, v, a in entries if n == "apple")
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "geosite_regex.json")
    with open(out, "w", encoding="utf-8") as f:
        json.dump({"entries": entries, "samples": samples, "extra": extra, "pinned": pinned}, f, indent=0,
                  ensure_ascii=True)
        f.write("\n")
    print("lists", len(lists), "regex entries", len(entries), "distinct", len(samples), "bytes", os.path.getsize(out))


if __name__ == "__main__":
    main(sys.argv[1])
