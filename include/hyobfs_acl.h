/*
 * hyobfs_acl.h -- the outbound ACL's rule matching (apernet/hysteria
 * extras/outbounds/acl), batched on the GPU: a batch of host names (as the
 * sniffer of hyobfs_sniff.h leaves them in device memory) and addresses in, one
 * routing decision per item out.
 *
 *   Go (reference)                                          C ABI
 *   ------------------------------------------------------  ----------------------------------------
 *   compiledRule{Outbound, HostMatcher, Protocol,           hyobfs_acl_rule (one per compiled rule)
 *     StartPort, EndPort, HijackAddress}  compile.go:53-60
 *   Compile(...) -> compiledRuleSetImpl   compile.go:130-161 hyobfs_acl_ruleset_new / _free / _rules
 *   (*compiledRuleSetImpl).Match          compile.go:88-109  hyobfs_acl_match_batch (device)
 *     (*compiledRule).Match               compile.go:62-70
 *   Sniffer.UDP / .TCP, then Match on the rewritten address  hyobfs_acl_match_sniffed_batch (device)
 *   allMatcher                            matchers.go:75-79  HYOBFS_ACL_ALL
 *   ipMatcher                             matchers.go:20-26  HYOBFS_ACL_IP
 *   cidrMatcher                           matchers.go:28-34  HYOBFS_ACL_CIDR
 *   domainMatcher, deepMatchRune          matchers.go:36-73  HYOBFS_ACL_DOMAIN_EXACT / _WILDCARD / _SUFFIX
 *   geositeMatcher               matchers_v2geo.go:114-161   HYOBFS_ACL_DOMAIN_SET
 *   geoipMatcher                 matchers_v2geo.go:16-60     HYOBFS_ACL_CIDR_SET
 *
 * Parsing the text rules (parse.go), compiling them (compile.go:130-326:
 * parseProtoPort, compileHostMatcher, the outbound and hijack lookups), reading
 * geoip / geosite files and applying a geosite rule's attribute filter
 * (matchers_v2geo.go:122-132) stay with the caller: a Go binding compiles as it
 * does today and hands each compiledRule over as one hyobfs_acl_rule.  The LRU
 * cache of compile.go:79,95-107 only remembers results and has no counterpart.
 *
 * THE MATCH RULES.  Per item, in the reference's order:
 *
 *    1. The name is lower-cased (ASCII 'A'-'Z') and every trailing '.' is
 *       removed (compile.go:89).  A name that is only dots becomes empty.
 *    2. The rules are tried in order; the first that matches decides
 *       (compile.go:98-104).  A rule matches when
 *         a. its proto is 0 or equals the item's (compile.go:63),
 *         b. its start_port is 0, or start_port <= port <= end_port (:66), and
 *         c. its host matcher matches (:69), by the rules below.
 *    3. No rule matches: rule = -1 (the reference returns the zero outbound,
 *       "use the default").
 *
 *   ALL              always.
 *   IP               net.IP.Equal(rule, IPv4) || net.IP.Equal(rule, IPv6).
 *                    TRAP 1: Equal treats an IPv4 address and its v4-mapped
 *                    IPv6 form (::ffff:a.b.c.d) as equal, in both directions;
 *                    an absent address equals nothing.
 *   CIDR             IPNet.Contains(IPv4) || IPNet.Contains(IPv6).
 *                    TRAP 2: Contains first reduces both the network address
 *                    and the IP with To4 (a 4-byte address, or a 16-byte one
 *                    that is v4-mapped, becomes 4 bytes), then requires equal
 *                    lengths, then compares under the mask.  So a v4 network
 *                    contains a v4-mapped IPv6 host address, and a true IPv6
 *                    network never contains an IPv4 one.
 *                    TRAP 3: a family-6 network whose address is v4-mapped is
 *                    reduced to 4 bytes and compared under the LAST FOUR bytes
 *                    of its 16-byte mask (net.networkNumberAndMask takes
 *                    m[12:] and does not look at the first twelve).  With a
 *                    prefix of 96 or more that is the v4 network of
 *                    prefix - 96 bits.  With a prefix below 96 those four mask
 *                    bytes are zero: the network contains every IPv4 (and
 *                    v4-mapped) address and no true IPv6 one.  (Go's
 *                    ParseCIDR never produces the latter, because it masks
 *                    the address first and the result is no longer v4-mapped;
 *                    a hand-built IPNet can.)
 *   DOMAIN_EXACT     name == pattern.
 *   DOMAIN_SUFFIX    name == pattern, or name ends with "." + pattern
 *                    ("fakenews.com" does not match "news.com").
 *   DOMAIN_WILDCARD  deepMatchRune (matchers.go:58-73): '*' in the pattern
 *                    matches any run of characters, the empty one included;
 *                    every other pattern character matches itself; the whole
 *                    name must be consumed.  The device uses the iterative
 *                    form that remembers the last '*' and backtracks to it,
 *                    which accepts the same pairs in O(name x pattern) steps.
 *   DOMAIN_SET       any entry matches (matchers_v2geo.go:154-161):
 *                    FULL name == value; ROOT name == value or name ends with
 *                    "." + value; PLAIN value is a substring of name (the empty
 *                    value always is).  The attribute filter has been applied
 *                    by the caller: only the entries that pass it are handed
 *                    over.  REGEX: regexp.MatchString(value, name)
 *                    (matchers_v2geo.go:137-140, :173-182), for a value inside
 *                    THE REGEX SUBSET below and a rule set made by
 *                    hyobfs_acl_ruleset_new_flags with HYOBFS_ACL_FLAG_REGEX;
 *                    every other REGEX entry is refused at creation
 *                    (HYOBFS_ACL_ERR_REGEX).  The set's result does not depend
 *                    on the order of its entries, and the device keeps a rule's
 *                    REGEX entries together after its other entries, so that
 *                    their walks run side by side in as few 64-entry steps as
 *                    possible.
 *   CIDR_SET         geoipMatcher.Match (matchers_v2geo.go:48-60): matchIP of
 *                    IPv4 if present, then of IPv6 if present; a hit returns
 *                    !inverse, no hit (also: no address at all) returns
 *                    inverse.  matchIP (:24-46) reduces the IP with To4 and
 *                    picks the family-4 list for a 4-byte result, else the
 *                    family-6 list, and runs exactly this binary search over
 *                    the list sorted by entry address:
 *                        left, right = 0, len - 1
 *                        while left <= right:
 *                            mid = (left + right) / 2
 *                            if entry[mid] Contains ip: return true
 *                            if entry[mid].address < ip (bytes.Compare): left = mid + 1
 *                            else: right = mid - 1
 *                    The comparison uses the entry's address AS GIVEN, not
 *                    masked, so an entry whose address lies above its network
 *                    address can hide a range from the search; that is the
 *                    reference's behaviour and it is kept.  Overlapping
 *                    entries are likewise found or not as this search goes.
 *
 * The domain matchers see the name after idna.ToUnicode (matchers.go:42-45),
 * the set matchers see it as it is.  Two facts let the device skip ToUnicode:
 *   FACT 1.  For a name that is all ASCII and does not contain "xn--",
 *            ToUnicode is the identity: it only rewrites labels that begin
 *            with "xn--".
 *   FACT 2.  For an all-ASCII name, matching bytes equals matching runes
 *            (deepMatchRune over []rune): every rune of the name is one byte,
 *            and a multi-byte rune of the pattern can equal none of them in
 *            either form.
 * NAMES LEFT TO THE HOST.  An item whose name holds a byte >= 0x80, or the
 * substring "xn--" anywhere after lower-casing, or is longer than
 * HYOBFS_ACL_MAX_NAME bytes as given, gets HYOBFS_ACL_ERR_HOST and the device
 * decides nothing for it, whatever the rules are; the caller matches it itself
 * (hysteria_amd/acl.py does).
 *
 * THE REGEX SUBSET.  The device compiles a REGEX value into a DFA over bytes
 * (hysteria_amd/csrc/acl_regex.h) and takes it only if every construct in it is
 * of this list; anything else is refused and never guessed at.  The Go binding
 * has already run regexp.Compile, so a value that is invalid in Go never arrives:
 * the device only decides between "mine" and "not mine".
 *   - literals; '\' followed by a non-alphanumeric ASCII byte, which is that byte
 *   - \d \D \w \W \s \S, inside classes as well
 *   - '.'
 *   - [...] and [^...] with single bytes, ranges and the escapes above
 *   - ( ) and (?: )
 *   - '|'; empty branches are allowed ("a|" matches everything, as in Go)
 *   - * + ? {n} {n,} {n,m} with n, m <= 1000, each optionally followed by one
 *     lazy '?', which is ignored: laziness does not change whether a match exists
 *   - '^' and '$' anywhere
 * Refused with HYOBFS_ACL_ERR_REGEX:
 *   - any other (?...) form: flags, named groups
 *   - \b \B \A \z \pX \Q \x.. and every other alphanumeric escape; a
 *     backslash at the end
 *   - POSIX [[:...:]] or a '[' inside a class; ']' as the first class member; a
 *     range that runs backwards or ends in a class escape; an unclosed class
 *   - a '{' that is not one of the three valid repeat forms (Go reads "a{,3}" as
 *     literal text, Python as {0,3}), m < n, a count above 1000; a '}' or a ']'
 *     that closes nothing (write "\}" and "\]")
 *   - a repeat applied to a repeat, to an anchor or to nothing
 *   - an unclosed group, a stray ')', groups nested more than 64 deep
 *   - a pattern byte >= 0x80
 *   - a DFA of more than HYOBFS_ACL_REGEX_MAX_STATES states ("a.{12}b$" is
 *     refused for this reason), or counted repeats that expand to more than
 *     65536 NFA states
 * A value longer than HYOBFS_ACL_MAX_NAME stays HYOBFS_ACL_ERR_PATTERN.
 * Semantics (Go regexp, no flags): the match is unanchored on both sides unless
 * the pattern anchors it; '^' is the beginning of the text and '$' its end (no
 * multi-line mode); '.' is every byte but '\n'; \s is [\t\n\f\r ]; \w is
 * [0-9A-Za-z_].  The name is the normalised one of rule 1, as for every other
 * DOMAIN_SET entry; the pattern is NOT lower-cased, so an upper-case literal
 * simply never matches.  An empty pattern matches every name; an empty name is
 * a name.
 *   TRAP a: Go's \s excludes \v (0x0b); Python's includes it.
 *   TRAP b: Go's '$' does not match before a trailing '\n'; Python's does
 *           (Python's \Z is Go's '$').
 *   TRAP c: at position 0 of an empty name both '^' and '$' hold, so "$^" and
 *           "^$" match the empty name and nothing else: the start state's
 *           end-of-text transition is computed with both assertions true.
 *   TRAP d: '^' after a consumed byte never holds: "a^b" compiles to a DFA that
 *           never accepts.
 * The names left to the host (below) are why the device may treat bytes as
 * runes: every name it matches is ASCII.
 *
 * THE INDEX.  A DOMAIN_SET of geosite size (cn: 65,029 entries) is too long to
 * walk entry by entry.  hyobfs_acl_ruleset_new_opts with HYOBFS_ACL_FLAG_INDEX
 * puts the FULL and ROOT values of a large enough set into a hash table on the
 * device and looks the name up instead.  The match rule, restated from
 * matchers_v2geo.go:141-147 for the normalised name of rule 1 (length nl):
 *   FULL v  matches iff name == v.
 *   ROOT v  matches iff name == v, or there is an i >= 1 with name[i-1] == '.'
 *           and name[i:] == v.
 * So the candidates of a name are its whole text (for FULL and ROOT values) and
 * every suffix that begins right after a '.' (for ROOT values only): at most 128
 * for a name of 255 bytes.  Each candidate is looked up; a hash hit is never a
 * match by itself, the value's bytes are compared, all of them.  The rule has no
 * exceptions: ROOT ".b" matches "a..b"; ROOT "value" matches ".value"; ROOT ""
 * and FULL "" match the empty name and nothing else (a normalised name does not
 * end in '.'); a value with an upper-case letter, a byte >= 0x80, "xn--" or a
 * trailing dot matches no name the device decides.  A set's result does not
 * depend on the order of its entries, so "some indexed value matches" is the
 * predicate of the linear walk over the same values: THE INDEX CHANGES NO
 * RESULT, only the time a large set takes.  Duplicate values are merged; a value
 * given as FULL and as ROOT is one value of both types.  PLAIN and REGEX entries
 * of an indexed set stay entries of the walk, after the set's index; the rule's
 * proto and ports gate the index as they gate every entry.  The rules
 * DOMAIN_EXACT / _SUFFIX / _WILDCARD are never indexed.
 * What counts toward index_min: the set's entries of type FULL or ROOT as given
 * (duplicates included; PLAIN and REGEX entries do not count).
 *
 * STATED DIVERGENCE.  The reference sorts a CIDR set with sort.Slice, which is
 * not stable, so the order of entries with equal addresses is unspecified
 * there.  Here the sort is stable by address bytes with the shorter prefix
 * first among equal addresses.
 *
 * Plain C ABI: pointers, sizes, integer status codes.  Additive to ABI 4.
 */
#ifndef HYOBFS_ACL_H
#define HYOBFS_ACL_H

#include <stddef.h>
#include <stdint.h>

#include "hyobfs.h"
#include "hyobfs_sniff.h"

#ifdef __cplusplus
extern "C" {
#endif

/* longest name the device matches and longest pattern / set value a rule may carry */
#define HYOBFS_ACL_MAX_NAME 255

/* per-item and creation status, continuing after HYOBFS_SNIFF_ERR_* */
#define HYOBFS_ACL_ERR_NO_NAME (-61)  /* match_sniffed: sres[i].status != OK or name_len == 0 */
#define HYOBFS_ACL_ERR_HOST (-62)     /* the name is left to the host (see above) */
#define HYOBFS_ACL_ERR_REGEX (-63)    /* a DOMAIN_SET entry of type REGEX that the device does not take */
#define HYOBFS_ACL_ERR_PATTERN (-64)  /* ruleset_new: a pattern or set value longer than HYOBFS_ACL_MAX_NAME */

#define HYOBFS_ACL_NO_HIJACK 0xFFFFFFFFu

enum {
    HYOBFS_ACL_ALL = 0,             /* allMatcher */
    HYOBFS_ACL_IP = 1,              /* ipMatcher: addr, family */
    HYOBFS_ACL_CIDR = 2,            /* cidrMatcher: addr, family, prefix */
    HYOBFS_ACL_DOMAIN_EXACT = 3,    /* domainMatcher, domainMatchExact: pattern */
    HYOBFS_ACL_DOMAIN_WILDCARD = 4, /* domainMatchWildcard */
    HYOBFS_ACL_DOMAIN_SUFFIX = 5,   /* domainMatchSuffix */
    HYOBFS_ACL_DOMAIN_SET = 6,      /* geositeMatcher: entries -> hyobfs_acl_domain[n_entries] */
    HYOBFS_ACL_CIDR_SET = 7         /* geoipMatcher: entries -> hyobfs_acl_cidr[n_entries], inverse */
};

/* geositeDomainType (matchers_v2geo.go:100-105) */
enum { HYOBFS_ACL_DOMAIN_PLAIN = 0, HYOBFS_ACL_DOMAIN_REGEX = 1, HYOBFS_ACL_DOMAIN_ROOT = 2, HYOBFS_ACL_DOMAIN_FULL = 3 };

/* one geositeDomain that passed the rule's attribute filter */
typedef struct hyobfs_acl_domain {
    uint32_t type; /* HYOBFS_ACL_DOMAIN_* */
    uint32_t len;
    const uint8_t* value; /* len bytes, lower case as the database has them; may be null when len == 0 */
} hyobfs_acl_domain;      /* 16 bytes */

/* one v2geo CIDR (matchers_v2geo.go:65-80): family 4 = addr[0, 4) and a prefix
   of at most 32, family 6 = addr[0, 16) and a prefix of at most 128.  The
   address bytes are taken as given (not masked). */
typedef struct hyobfs_acl_cidr {
    uint8_t addr[16];
    uint8_t family;
    uint8_t prefix;
    uint8_t pad_[2];
} hyobfs_acl_cidr; /* 20 bytes */

/* one compiledRule (compile.go:53-60) */
typedef struct hyobfs_acl_rule {
    uint32_t kind;          /* HYOBFS_ACL_* */
    uint32_t proto;         /* Protocol: 0 both, 1 TCP, 2 UDP (compile.go:16-20) */
    uint16_t start_port;    /* 0 = any port */
    uint16_t end_port;
    uint32_t outbound;      /* the caller's, copied to the result */
    uint32_t hijack;        /* index into a table of the caller's, or HYOBFS_ACL_NO_HIJACK */
    uint32_t pattern_len;   /* DOMAIN_EXACT / _WILDCARD / _SUFFIX */
    const uint8_t* pattern; /* lower case, no trailing dots (compile.go:236) */
    uint8_t addr[16];       /* IP / CIDR: family 4 = addr[0, 4), family 6 = addr[0, 16) */
    uint8_t family;         /* 4 or 6: the length of the reference's net.IP (4 or 16 bytes) */
    uint8_t prefix;         /* CIDR: ones in the mask, of 32 (family 4) or 128 (family 6) bits */
    uint8_t inverse;        /* CIDR_SET: GeoIP.InverseMatch */
    uint8_t pad_;
    uint32_t n_entries;     /* DOMAIN_SET / CIDR_SET */
    const void* entries;    /* hyobfs_acl_domain[] or hyobfs_acl_cidr[]; may be null when n_entries == 0 */
} hyobfs_acl_rule;          /* 64 bytes */

typedef struct hyobfs_acl_ruleset hyobfs_acl_ruleset;

/*
 * Validates the rules, brings them into the device's form (CIDR sets sorted as
 * stated above) and uploads them to `device` once.  Never launches a kernel.
 * The rules and everything they point to may be freed after the call.  Refusals,
 * checked for every rule before the device is looked at: an unknown kind,
 * proto > 2, a bad family or a prefix beyond it, a null pattern with a non-zero
 * length or null entries with a non-zero count (HYOBFS_ERR_INVALID; a domain
 * rule's pattern must not be null at all); a REGEX entry, whatever its value
 * (HYOBFS_ACL_ERR_REGEX; hyobfs_acl_ruleset_new_flags takes them); a pattern or value longer than HYOBFS_ACL_MAX_NAME
 * (HYOBFS_ACL_ERR_PATTERN).  hyobfs_acl_ruleset_bad_rule() then names the rule.
 * n_rules == 0 is valid (rules may be null): every item gets rule = -1.
 */
int hyobfs_acl_ruleset_new(const hyobfs_acl_rule* rules, uint32_t n_rules, int device, hyobfs_acl_ruleset** out);

/* hyobfs_acl_ruleset_new_flags: REGEX entries inside the subset are compiled and matched on the device */
#define HYOBFS_ACL_FLAG_REGEX 1u
/* the largest DFA a REGEX entry may compile to */
#define HYOBFS_ACL_REGEX_MAX_STATES 4096

/*
 * hyobfs_acl_ruleset_new with flags; flags == 0 is that call.  With
 * HYOBFS_ACL_FLAG_REGEX every REGEX entry is compiled (THE REGEX SUBSET above);
 * the first one the device cannot take gives HYOBFS_ACL_ERR_REGEX, checked like
 * every other refusal before the device is looked at:
 * hyobfs_acl_ruleset_bad_rule() names the rule and hyobfs_acl_ruleset_bad_entry()
 * the entry within it.  Unknown flag bits: HYOBFS_ERR_INVALID.
 */
int hyobfs_acl_ruleset_new_flags(const hyobfs_acl_rule* rules, uint32_t n_rules, int device, uint32_t flags,
                                 hyobfs_acl_ruleset** out);

/* hyobfs_acl_options.flags only (hyobfs_acl_ruleset_new_flags refuses it): THE INDEX above */
#define HYOBFS_ACL_FLAG_INDEX 2u
/* more FULL + ROOT values than one 64-entry step of the walk holds */
#define HYOBFS_ACL_INDEX_MIN_DEFAULT 65u

typedef struct hyobfs_acl_options {
    uint32_t struct_size; /* sizeof(hyobfs_acl_options); anything else: HYOBFS_ERR_INVALID */
    uint32_t flags;       /* HYOBFS_ACL_FLAG_REGEX | HYOBFS_ACL_FLAG_INDEX; other bits: HYOBFS_ERR_INVALID */
    uint32_t index_min;   /* with FLAG_INDEX: a DOMAIN_SET with at least this many FULL + ROOT entries is
                             indexed; 0 = HYOBFS_ACL_INDEX_MIN_DEFAULT; 1 = every set that has one.
                             Without FLAG_INDEX it must be 0 */
    uint32_t reserved;    /* 0 */
} hyobfs_acl_options;     /* 16 bytes */

/*
 * hyobfs_acl_ruleset_new with options; opts == NULL is that call.  The options
 * are checked first (HYOBFS_ERR_INVALID, bad_rule() == -1), then the rules as by
 * hyobfs_acl_ruleset_new_flags with the REGEX bit of opts->flags, all before the
 * device is looked at; hyobfs_acl_ruleset_bad_rule() and _bad_entry() name rule
 * and entry as there (an indexed value longer than HYOBFS_ACL_MAX_NAME is
 * HYOBFS_ACL_ERR_PATTERN like any other).  With HYOBFS_ACL_FLAG_INDEX every
 * DOMAIN_SET that reaches index_min gets an index (THE INDEX above, which also
 * says what counts); every other set, and every set without the flag, is
 * compiled exactly as by the other two calls.  The index changes no result.
 */
int hyobfs_acl_ruleset_new_opts(const hyobfs_acl_rule* rules, uint32_t n_rules, int device,
                                const hyobfs_acl_options* opts, hyobfs_acl_ruleset** out);
void hyobfs_acl_ruleset_free(hyobfs_acl_ruleset* set);
uint32_t hyobfs_acl_ruleset_rules(const hyobfs_acl_ruleset* set);
/* entries of the table the kernel walks, 64 per step: an indexed set counts one for its index and
   one for each of its PLAIN and REGEX entries; 0 for a null set */
uint32_t hyobfs_acl_ruleset_entries(const hyobfs_acl_ruleset* set);

typedef struct hyobfs_acl_index_info {
    uint32_t values;    /* distinct FULL / ROOT values in the table */
    uint32_t slots;     /* power of two, at least 2 * values; 0 = this rule has no index */
    uint32_t max_probe; /* longest probe sequence of any stored value, in slots looked at (1: none collided) */
    uint32_t reserved;
} hyobfs_acl_index_info;
/* the index of rule `rule`, all zero if it has none; a null pointer or rule >= the rule count:
   HYOBFS_ERR_INVALID */
int hyobfs_acl_ruleset_index_info(const hyobfs_acl_ruleset* set, uint32_t rule, hyobfs_acl_index_info* out);
/* index of the rule that this thread's last failed hyobfs_acl_ruleset_new refused, or -1 */
int64_t hyobfs_acl_ruleset_bad_rule(void);
/* index, within that rule's entries as given, of the DOMAIN_SET entry that was refused; -1 when the
   refusal was not about one entry */
int64_t hyobfs_acl_ruleset_bad_entry(void);

/*
 * Host only, no device.  Whether the device takes this REGEX value: HYOBFS_OK
 * (and, where the pointers are not null, the states of its DFA's subset
 * construction and its byte classes), HYOBFS_ACL_ERR_REGEX, HYOBFS_ACL_ERR_PATTERN
 * or HYOBFS_ERR_INVALID (a null pattern with a length).  A binding asks per
 * entry and keeps on the host only a rule that holds a refused value.
 */
int hyobfs_acl_regex_check(const uint8_t* pattern, uint32_t len, uint32_t* n_states, uint32_t* n_classes);

/*
 * Host only: the scalar counterpart of the kernel's REGEX entry.  Compiles the
 * value, then runs the walk the kernel runs over name[0, name_len) AS GIVEN
 * (not normalised; any bytes, any length): 1 match, 0 none, or a negative
 * status as hyobfs_acl_regex_check gives it.
 */
int hyobfs_acl_regex_match(const uint8_t* pattern, uint32_t len, const uint8_t* name, uint32_t name_len);

typedef struct hyobfs_acl_result {
    int32_t status;    /* HYOBFS_OK, HYOBFS_ACL_ERR_NO_NAME or HYOBFS_ACL_ERR_HOST */
    int32_t rule;      /* index of the first matching rule; -1: none, or status != OK */
    uint32_t outbound; /* of that rule; 0 when rule == -1 */
    uint32_t hijack;   /* of that rule; HYOBFS_ACL_NO_HIJACK when rule == -1 */
} hyobfs_acl_result;   /* 16 bytes */

/*
 * The two batched calls share these rules.  All arrays are device memory of
 * the rule set's device; calls are asynchronous on `stream`; a rule set may be
 * used by any number of calls and streams at once (it is read-only).  n == 0
 * returns HYOBFS_OK; a null required pointer returns HYOBFS_ERR_INVALID.
 * ipv4 is 4 bytes per item, ipv6 16; bit 0 / bit 1 of ip_flags[i] say whether
 * item i has the one / the other (HostInfo.IPv4 / IPv6 nil or not); ip_flags
 * null means no item has an address, and only then may ipv4 and ipv6 be null
 * (they are not read).  proto is one byte per item (0, 1 TCP, 2 UDP), port a
 * uint16 per item.
 * Exactly res[0, n) is written and nothing else.
 */

/* Match over names[name_off[i], +name_len[i]); an empty name is a name. */
int hyobfs_acl_match_batch(const hyobfs_acl_ruleset* set, const uint8_t* names, const uint64_t* name_off,
                           const uint32_t* name_len, const uint8_t* ipv4, const uint8_t* ipv6, const uint8_t* ip_flags,
                           const uint8_t* proto, const uint16_t* port, uint64_t n, hyobfs_acl_result* res,
                           void* stream);

/*
 * Match over names[i * name_stride, +sres[i].name_len), exactly as the three
 * calls of hyobfs_sniff.h leave names and sres.  An item whose sres[i].status
 * is not HYOBFS_OK or whose name_len is 0 gets HYOBFS_ACL_ERR_NO_NAME and
 * nothing of its name row is read: that request keeps its own address, which
 * the caller matches itself.
 */
int hyobfs_acl_match_sniffed_batch(const hyobfs_acl_ruleset* set, const uint8_t* names, uint32_t name_stride,
                                   const hyobfs_sniff_result* sres, const uint8_t* ipv4, const uint8_t* ipv6,
                                   const uint8_t* ip_flags, const uint8_t* proto, const uint16_t* port, uint64_t n,
                                   hyobfs_acl_result* res, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HYOBFS_ACL_H */
