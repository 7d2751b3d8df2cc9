// acl_regex.h -- a geosite entry of type regex as a DFA: the host compiler and the
// scalar walk that the kernel, the emulation and the host share
// (include/hyobfs_acl.h, "THE REGEX SUBSET", states what is taken and what it means).
//
// Reference: geositeMatcher.matchDomain (matchers_v2geo.go:137-140, :173-182):
// regexp.Compile(value), then Regex.MatchString(host.Name).  A boolean MatchString
// over the subset is a DFA run: nothing in it needs backtracking.
//
//   parse     recursive descent into a small AST; everything outside the subset is
//             refused, never guessed at
//   NFA       Thompson's construction; counted repeats are expanded; '^' and '$'
//             are assertion edges
//   DFA       subset construction over byte classes (bytes that no transition of
//             the NFA tells apart are tried once) plus one end-of-text column.
//             The match is unanchored, so the NFA's start is re-entered after
//             every byte, and sticky, so a set that holds the accepting state IS
//             the reserved id kAccept.  A state that cannot reach kAccept is the
//             reserved id kDead.  The start state is the only one at which '^'
//             holds; it is never merged with a later state, and its end-of-text
//             column is computed with '^' and '$' both true (hyobfs_acl.h, trap c).
//
// The device form of one regex: rows x kCols uint16 cells.  Cell [s][b] is the state
// after the ASCII byte b; cell [s][128] the state after any byte >= 0x80 (a pattern
// has no such byte, so every set holds all of them or none: they are one class);
// cell [s][129] the verdict at the end of the text (kAccept or kDead).  The start
// state (0, kAccept or kDead) is kept by the caller.  One load a byte: the first
// layout, a 256-byte class map in front of rows of classes + 1 cells, was a sixth
// of the size and two dependent loads a byte, and a regex-bearing step cost 12-15 us
// per wave against 7-9 us with a column per byte.
#ifndef HYOBFS_ACL_REGEX_H
#define HYOBFS_ACL_REGEX_H

#include <algorithm>
#include <bitset>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "kernels.h"

namespace hyobfs {
namespace acl {
namespace rx {

constexpr uint32_t kAccept = 0xFFFF, kDead = 0xFFFE;
constexpr uint32_t kHigh = 128, kEnd = 129, kCols = 130;   // the columns after the 128 ASCII ones
constexpr uint32_t kMaxStates = 4096;      // HYOBFS_ACL_REGEX_MAX_STATES
constexpr uint32_t kMaxRepeat = 1000;
constexpr uint32_t kMaxNfa = 1u << 16;     // expanded repeats beyond this are refused
constexpr uint32_t kMaxDepth = 64;         // nested groups

// MatchString over name[0, nl): one dependent load a byte, left at kAccept or kDead.
HY_HD bool walk(const uint16_t* cells, uint32_t start, const uint8_t* name, uint32_t nl) {
    uint32_t s = start;
    for (uint32_t i = 0; i < nl && s < kDead; ++i) {
        const uint32_t b = name[i];
        s = cells[s * kCols + (b < kHigh ? b : kHigh)];
    }
    if (s >= kDead) return s == kAccept;
    return cells[s * kCols + kEnd] == kAccept;
}

// ---- host: the compiler
using ByteSet = std::bitset<256>;

struct Node {
    enum Kind : uint8_t { kSet, kBol, kEol, kCat, kAlt, kRep } kind;
    ByteSet set;                  // kSet
    std::vector<uint32_t> kids;   // kCat, kAlt; kRep: one
    uint32_t lo = 0, hi = 0;      // kRep; hi == ~0u: no upper bound
};

struct Dfa {
    uint32_t start = kDead, states = 0, classes = 0;
    std::vector<uint16_t> cells;   // the device form
};

class Compiler {
  public:
    // false: the pattern is not in the subset, or its DFA is too large
    bool compile(const uint8_t* p, uint32_t len, Dfa& out) {
        p_ = p;
        n_ = len;
        for (uint32_t k = 0; k < len; ++k)
            if (p[k] >= 0x80) return false;
        uint32_t root;
        if (!alt(root, 0) || at_ != n_) return false;   // a stray ')'
        uint32_t s, e;
        if (!build(root, s, e)) return false;
        return subsets(s, e, out);
    }

  private:
    // -- the parser
    const uint8_t* p_ = nullptr;
    uint32_t n_ = 0, at_ = 0;
    std::vector<Node> ast_;

    int peek() const { return at_ < n_ ? p_[at_] : -1; }
    uint32_t node(Node::Kind k) {
        ast_.emplace_back();
        ast_.back().kind = k;
        return (uint32_t)ast_.size() - 1;
    }
    static bool alnum(int c) { return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }
    static ByteSet range(uint32_t lo, uint32_t hi) {
        ByteSet s;
        for (uint32_t b = lo; b <= hi; ++b) s.set(b);
        return s;
    }
    // after the backslash: a Perl class or an escaped punctuation byte
    bool escape(ByteSet& s, bool& single) {
        const int c = peek();
        if (c < 0) return false;
        ++at_;
        single = !alnum(c);
        s.reset();
        if (single) {
            s.set((size_t)c);
            return true;
        }
        switch (c) {
            case 'd': case 'D': s = range('0', '9'); break;
            case 'w': case 'W': s = range('0', '9') | range('a', 'z') | range('A', 'Z'); s.set('_'); break;
            case 's': case 'S': s.set('\t'); s.set('\n'); s.set('\f'); s.set('\r'); s.set(' '); break;   // no \v: trap a
            default: return false;   // \b \B \A \z \p \Q \x, a back-reference, ...
        }
        if (c < 'a') s = ~s;
        return true;
    }
    bool char_class(ByteSet& out) {   // after '['
        bool neg = false;
        if (peek() == '^') {
            neg = true;
            ++at_;
        }
        ByteSet s;
        for (bool first = true;; first = false) {
            int c = peek();
            if (c < 0 || c == '[') return false;       // unclosed; POSIX or a '[' in a class
            if (c == ']') {
                if (first) return false;               // ']' as the first member
                ++at_;
                break;
            }
            ++at_;
            ByteSet one;
            bool single = true;
            if (c == '\\') {
                if (!escape(one, single)) return false;
                if (!single) {
                    s |= one;
                    continue;
                }
                for (c = 0; !one.test((size_t)c); ++c) {}
            }
            if (peek() == '-' && at_ + 1 < n_ && p_[at_ + 1] != ']') {
                ++at_;
                int h = p_[at_++];
                if (h == '[') return false;
                if (h == '\\') {
                    if (!escape(one, single) || !single) return false;   // a range up to a class
                    for (h = 0; !one.test((size_t)h); ++h) {}
                }
                if (h < c) return false;
                s |= range((uint32_t)c, (uint32_t)h);
            } else {
                s.set((size_t)c);
            }
        }
        out = neg ? ~s : s;
        return true;
    }
    bool atom(uint32_t& out, uint32_t depth) {
        const int c = peek();
        if (c == '(') {
            ++at_;
            if (peek() == '?') {
                if (at_ + 1 < n_ && p_[at_ + 1] == ':') at_ += 2;
                else return false;   // flags, named groups
            }
            if (depth >= kMaxDepth || !alt(out, depth + 1) || peek() != ')') return false;
            ++at_;
            return true;
        }
        if (c == '*' || c == '+' || c == '?' || c == '{' || c == '}' || c == ']') return false;
        ++at_;
        if (c == '^' || c == '$') {
            out = node(c == '^' ? Node::kBol : Node::kEol);
            return true;
        }
        out = node(Node::kSet);
        if (c == '[') return char_class(ast_[out].set);
        if (c == '\\') {
            bool single;
            return escape(ast_[out].set, single);
        }
        if (c == '.') {
            ast_[out].set.set();
            ast_[out].set.reset('\n');
        } else {
            ast_[out].set.set((size_t)c);
        }
        return true;
    }
    bool number(uint32_t& v) {
        if (peek() < '0' || peek() > '9') return false;
        for (v = 0; peek() >= '0' && peek() <= '9'; ++at_) {
            v = v * 10 + (uint32_t)(peek() - '0');
            if (v > kMaxRepeat) return false;
        }
        return true;
    }
    bool repeat(uint32_t& out, uint32_t depth) {
        if (!atom(out, depth)) return false;
        const int c = peek();
        uint32_t lo, hi;
        if (c == '*' || c == '+' || c == '?') {
            ++at_;
            lo = c == '+';
            hi = c == '?' ? 1 : ~0u;
        } else if (c == '{') {   // {n} {n,} {n,m} and nothing else
            ++at_;
            if (!number(lo)) return false;
            hi = lo;
            if (peek() == ',') {
                ++at_;
                hi = ~0u;
                if (peek() != '}' && (!number(hi) || hi < lo)) return false;
            }
            if (peek() != '}') return false;
            ++at_;
        } else {
            return true;
        }
        if (ast_[out].kind == Node::kBol || ast_[out].kind == Node::kEol) return false;   // a repeated anchor
        if (peek() == '?') ++at_;                                                          // lazy: the same language
        const int d = peek();
        if (d == '*' || d == '+' || d == '?' || d == '{') return false;                    // a repeated repeat
        const uint32_t r = node(Node::kRep);
        ast_[r].kids.push_back(out);
        ast_[r].lo = lo;
        ast_[r].hi = hi;
        out = r;
        return true;
    }
    bool alt(uint32_t& out, uint32_t depth) {
        std::vector<uint32_t> alts;
        for (;;) {
            std::vector<uint32_t> items;
            while (peek() >= 0 && peek() != '|' && peek() != ')') {
                uint32_t it;
                if (!repeat(it, depth)) return false;
                items.push_back(it);
            }
            const uint32_t c = node(Node::kCat);
            ast_[c].kids = std::move(items);
            alts.push_back(c);
            if (peek() != '|') break;
            ++at_;
        }
        out = node(Node::kAlt);
        ast_[out].kids = std::move(alts);
        return true;
    }

    // -- the NFA: per state at most one byte transition, any number of empty and assertion edges
    struct State {
        int32_t set = -1;   // index into sets_, or none
        uint32_t to = 0;
        std::vector<uint32_t> eps, bol, eol;
    };
    std::vector<State> nfa_;
    std::vector<ByteSet> sets_;

    bool fresh(uint32_t& s) {
        if (nfa_.size() >= kMaxNfa) return false;
        nfa_.emplace_back();
        s = (uint32_t)nfa_.size() - 1;
        return true;
    }
    uint32_t set_index(const ByteSet& b) {
        for (uint32_t k = 0; k < sets_.size(); ++k)
            if (sets_[k] == b) return k;
        sets_.push_back(b);
        return (uint32_t)sets_.size() - 1;
    }
    bool build(uint32_t n, uint32_t& s, uint32_t& e) {
        const Node::Kind kind = ast_[n].kind;
        if (kind == Node::kSet || kind == Node::kBol || kind == Node::kEol) {
            if (!fresh(s) || !fresh(e)) return false;
            if (kind == Node::kSet) {
                nfa_[s].set = (int32_t)set_index(ast_[n].set);
                nfa_[s].to = e;
            } else {
                (kind == Node::kBol ? nfa_[s].bol : nfa_[s].eol).push_back(e);
            }
            return true;
        }
        if (kind == Node::kCat) {
            if (!fresh(s)) return false;
            e = s;
            for (size_t k = 0; k < ast_[n].kids.size(); ++k) {
                uint32_t s2, e2;
                if (!build(ast_[n].kids[k], s2, e2)) return false;
                nfa_[e].eps.push_back(s2);
                e = e2;
            }
            return true;
        }
        if (kind == Node::kAlt) {
            if (!fresh(s) || !fresh(e)) return false;
            for (size_t k = 0; k < ast_[n].kids.size(); ++k) {
                uint32_t s2, e2;
                if (!build(ast_[n].kids[k], s2, e2)) return false;
                nfa_[s].eps.push_back(s2);
                nfa_[e2].eps.push_back(e);
            }
            return true;
        }
        // kRep: lo copies, then a loop or hi - lo optional copies
        const uint32_t x = ast_[n].kids[0], lo = ast_[n].lo, hi = ast_[n].hi;
        if (!fresh(s)) return false;
        e = s;
        for (uint32_t k = 0; k < lo; ++k) {
            uint32_t s2, e2;
            if (!build(x, s2, e2)) return false;
            nfa_[e].eps.push_back(s2);
            e = e2;
        }
        uint32_t end;
        if (!fresh(end)) return false;
        if (hi == ~0u) {
            uint32_t loop, s2, e2;
            if (!fresh(loop) || !build(x, s2, e2)) return false;
            nfa_[e].eps.push_back(loop);
            nfa_[loop].eps.push_back(s2);
            nfa_[e2].eps.push_back(loop);
            nfa_[loop].eps.push_back(end);
        } else {
            for (uint32_t k = lo; k < hi; ++k) {
                uint32_t s2, e2;
                nfa_[e].eps.push_back(end);
                if (!build(x, s2, e2)) return false;
                nfa_[e].eps.push_back(s2);
                e = e2;
            }
            nfa_[e].eps.push_back(end);
        }
        e = end;
        return true;
    }

    // -- the DFA
    std::vector<uint32_t> mark_;
    uint32_t epoch_ = 0;

    // `set` closed under the empty edges and the assertions that hold; sorted
    void closure(std::vector<uint32_t>& set, bool bol, bool eol) {
        if (mark_.size() != nfa_.size()) mark_.assign(nfa_.size(), 0);
        ++epoch_;
        std::vector<uint32_t> stack;
        for (uint32_t x : set)
            if (mark_[x] != epoch_) {
                mark_[x] = epoch_;
                stack.push_back(x);
            }
        set.clear();
        while (!stack.empty()) {
            const uint32_t x = stack.back();
            stack.pop_back();
            set.push_back(x);
            auto follow = [&](const std::vector<uint32_t>& edges) {
                for (uint32_t y : edges)
                    if (mark_[y] != epoch_) {
                        mark_[y] = epoch_;
                        stack.push_back(y);
                    }
            };
            follow(nfa_[x].eps);
            if (bol) follow(nfa_[x].bol);
            if (eol) follow(nfa_[x].eol);
        }
        std::sort(set.begin(), set.end());
    }
    static bool has(const std::vector<uint32_t>& set, uint32_t x) { return std::binary_search(set.begin(), set.end(), x); }

    bool subsets(uint32_t s0, uint32_t acc, Dfa& out) {
        // byte classes: two bytes that every transition set treats alike share a column
        uint8_t cls[256] = {};
        uint32_t n_cls = 1;
        for (const ByteSet& b : sets_) {
            std::map<std::pair<uint32_t, bool>, uint32_t> split;
            uint32_t next = 0;
            for (uint32_t c = 0; c < 256; ++c) {
                auto it = split.emplace(std::make_pair((uint32_t)cls[c], b.test(c)), next);
                if (it.second) ++next;
                cls[c] = (uint8_t)it.first->second;
            }
            n_cls = next;
        }
        uint8_t rep[256];
        for (uint32_t c = 256; c-- > 0;) rep[cls[c]] = (uint8_t)c;
        const uint32_t stride = n_cls + 1;

        std::vector<std::vector<uint32_t>> order;
        std::map<std::vector<uint32_t>, uint32_t> ids;   // every state but the start, which alone is at position 0
        std::vector<uint32_t> rows;                       // states x stride
        std::vector<uint32_t> cur{s0};
        closure(cur, true, false);
        out.classes = n_cls;
        out.cells.clear();
        if (has(cur, acc)) {   // the empty match: every name, the empty one too
            out.start = kAccept;
            out.states = 0;
            return true;
        }
        order.push_back(cur);
        for (uint32_t i = 0; i < order.size(); ++i) {
            rows.resize((size_t)(i + 1) * stride);
            for (uint32_t c = 0; c < n_cls; ++c) {
                std::vector<uint32_t> nxt{s0};   // unanchored: a match may begin after any byte
                for (uint32_t x : order[i])
                    if (nfa_[x].set >= 0 && sets_[(size_t)nfa_[x].set].test(rep[c])) nxt.push_back(nfa_[x].to);
                closure(nxt, false, false);
                uint32_t id = kAccept;
                if (!has(nxt, acc)) {
                    auto it = ids.find(nxt);
                    if (it == ids.end()) {
                        if (order.size() >= kMaxStates) return false;
                        it = ids.emplace(nxt, (uint32_t)order.size()).first;
                        order.push_back(std::move(nxt));
                    }
                    id = it->second;
                }
                rows[(size_t)i * stride + c] = id;
            }
            std::vector<uint32_t> end = order[i];
            closure(end, i == 0, true);   // trap c: at the start both assertions hold
            rows[(size_t)i * stride + n_cls] = has(end, acc) ? kAccept : kDead;
        }
        // dead states: those from which kAccept cannot be reached
        const uint32_t n = (uint32_t)order.size();
        std::vector<uint8_t> live(n, 0);
        std::vector<std::vector<uint32_t>> from(n);
        std::vector<uint32_t> todo;
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t c = 0; c < stride; ++c) {
                const uint32_t t = rows[(size_t)i * stride + c];
                if (t < kDead) {
                    from[t].push_back(i);
                } else if (t == kAccept && !live[i]) {
                    live[i] = 1;
                    todo.push_back(i);
                }
            }
        while (!todo.empty()) {
            const uint32_t t = todo.back();
            todo.pop_back();
            for (uint32_t i : from[t])
                if (!live[i]) {
                    live[i] = 1;
                    todo.push_back(i);
                }
        }
        std::vector<uint32_t> renum(n, kDead);
        uint32_t n_live = 0;
        for (uint32_t i = 0; i < n; ++i)
            if (live[i]) renum[i] = n_live++;
        out.states = n;
        out.start = renum[0];
        out.cells.assign((size_t)n_live * kCols, 0);
        for (uint32_t i = 0; i < n; ++i) {
            if (!live[i]) continue;
            for (uint32_t b = 0; b < kCols; ++b) {
                const uint32_t c = b == kEnd ? n_cls : cls[b == kHigh ? 0x80 : b];
                const uint32_t t = rows[(size_t)i * stride + c];
                out.cells[(size_t)renum[i] * kCols + b] = (uint16_t)(t < kDead ? renum[t] : t);
            }
        }
        return true;
    }
};

inline bool compile(const uint8_t* p, uint32_t len, Dfa& out) { return Compiler().compile(p, len, out); }

}  // namespace rx
}  // namespace acl
}  // namespace hyobfs
#endif  // HYOBFS_ACL_REGEX_H
