// filter.hip — what a WHERE predicate on the key columns region and product_id IS (contract in include/aqe_hip.h, the key
// predicate section; the reference filters in its SQL executor, executor.cpp:32-41, 68-92).  No kernel lives here.
//
// A key predicate is one more conjunct of the `pass` test a sweep applies per sampled row.  The host compiles each
// column's term into a DevTerm (key_term.hpp) — [lo, hi], a 64-bit word, a negate bit — that the device tests with two
// compares, a shift and an AND; an IN list over more than 64 consecutive keys keeps its 1024-bit map in LDS (16 words per
// column).  The sweep that applies the terms, and every aqe_*filtered* entry, is the power-sum sweep of moments.hip.  This
// file holds the term constructors, their compilation, the parser of a WHERE clause's key terms and the host-side test.
#include <cctype>

#include "host.hpp"
#include "key_term.hpp"

namespace aqe {

const char* term_defect(const aqe_key_term& t) {
    if (t.form < AQE_KEYTERM_NONE || t.form > AQE_KEYTERM_BITMAP) return "key term: form must be AQE_KEYTERM_NONE, _RANGE or _BITMAP";
    if (t.form == AQE_KEYTERM_BITMAP && (t.hi < t.lo || static_cast<int64_t>(t.hi) - t.lo >= AQE_KEY_BITMAP_BITS))
        return "key term: a bitmap covers 1 .. 1024 keys from its base";
    return nullptr;
}

void compile_term(const aqe_key_term& t, DevTerm* d, unsigned long long* map) {
    *d = pass_all();
    for (int i = 0; i < kMapWords; ++i) map[i] = 0;
    if (t.form == AQE_KEYTERM_NONE) return;
    d->lo = t.lo;
    d->hi = t.hi;
    d->negate = t.negate ? 1u : 0u;
    if (t.form == AQE_KEYTERM_BITMAP) {
        d->wide = static_cast<int64_t>(t.hi) - t.lo >= 64 ? 1u : 0u;
        d->bits0 = t.bits[0];
        for (int i = 0; i < kMapWords; ++i) map[i] = t.bits[i];
    }
}

namespace {

// ---- the WHERE clause's key terms (host) ----------------------------------------------------------------------------------

enum TokKind { T_IDENT, T_INT, T_NUMBER, T_OP, T_LP, T_RP, T_COMMA, T_OTHER };
struct Tok {
    TokKind kind;
    std::string text;  // identifiers in upper case
    size_t b, e;       // [b, e) of the query text
    long long ival;
};

std::vector<Tok> tokenize(const std::string& s) {
    std::vector<Tok> out;
    size_t i = 0;
    const size_t n = s.size();
    auto isid = [](char ch) { return std::isalnum(static_cast<unsigned char>(ch)) || ch == '_'; };
    while (i < n) {
        const char ch = s[i];
        if (std::isspace(static_cast<unsigned char>(ch))) { ++i; continue; }
        Tok t{T_OTHER, "", i, i + 1, 0};
        bool prev_value = false;  // a '-' behind a value is a minus, anywhere else the sign of a literal
        if (!out.empty()) {
            const Tok& b = out.back();
            const bool keyword = b.kind == T_IDENT && (b.text == "BETWEEN" || b.text == "AND" || b.text == "OR" || b.text == "NOT" || b.text == "IN" || b.text == "WHERE");
            prev_value = b.kind == T_INT || b.kind == T_NUMBER || b.kind == T_RP || (b.kind == T_IDENT && !keyword);
        }
        const bool digit = std::isdigit(static_cast<unsigned char>(ch));
        if (digit || ((ch == '-' || ch == '+') && !prev_value && i + 1 < n && std::isdigit(static_cast<unsigned char>(s[i + 1])))) {
            size_t j = i + (digit ? 0 : 1);
            while (j < n && std::isdigit(static_cast<unsigned char>(s[j]))) ++j;
            bool integer = true;
            if (j < n && s[j] == '.') { integer = false; ++j; while (j < n && std::isdigit(static_cast<unsigned char>(s[j]))) ++j; }
            if (j < n && (s[j] == 'e' || s[j] == 'E')) {
                size_t k = j + 1;
                if (k < n && (s[k] == '-' || s[k] == '+')) ++k;
                if (k < n && std::isdigit(static_cast<unsigned char>(s[k]))) { integer = false; j = k; while (j < n && std::isdigit(static_cast<unsigned char>(s[j]))) ++j; }
            }
            if (j < n && isid(s[j])) { integer = false; while (j < n && isid(s[j])) ++j; }  // 12abc: not a literal we take
            t.kind = integer ? T_INT : T_NUMBER;
            t.e = j;
            t.text = s.substr(i, j - i);
            if (integer) {
                const size_t digits = j - i - (digit ? 0 : 1);
                t.ival = digits > 12 ? (ch == '-' ? -(1ll << 40) : (1ll << 40)) : std::atoll(t.text.c_str());  // (far outside int32 either way)
            }
        } else if (std::isalpha(static_cast<unsigned char>(ch)) || ch == '_') {
            size_t j = i;
            while (j < n && (isid(s[j]) || s[j] == '.')) ++j;
            t.kind = T_IDENT;
            t.e = j;
            t.text = s.substr(i, j - i);
            for (char& c2 : t.text) c2 = static_cast<char>(std::toupper(static_cast<unsigned char>(c2)));
            const size_t dot = t.text.rfind('.');  // sales.region -> REGION
            if (dot != std::string::npos) t.text = t.text.substr(dot + 1);
        } else if (ch == '(') { t.kind = T_LP; }
        else if (ch == ')') { t.kind = T_RP; }
        else if (ch == ',') { t.kind = T_COMMA; }
        else if (ch == '<' || ch == '>' || ch == '=' || ch == '!') {
            size_t j = i + 1;
            if (j < n && (s[j] == '=' || (ch == '<' && s[j] == '>'))) ++j;
            t.kind = T_OP;
            t.e = j;
            t.text = s.substr(i, j - i);
        } else if (ch == '\'' || ch == '"') {
            size_t j = i + 1;
            while (j < n && s[j] != ch) ++j;
            t.e = j < n ? j + 1 : n;
            t.text = s.substr(i, t.e - i);
        } else {
            t.text = std::string(1, ch);
        }
        i = t.e;
        out.push_back(t);
    }
    return out;
}

int key_column_of(const Tok& t) {
    if (t.kind != T_IDENT) return 0;
    if (t.text == "REGION") return AQE_GROUP_REGION;
    if (t.text == "PRODUCT_ID") return AQE_GROUP_PRODUCT;
    return 0;
}

bool is_word(const Tok& t, const char* w) { return t.kind == T_IDENT && t.text == w; }

struct KeyParse {
    const std::string& src;
    const std::vector<Tok>& tk;
    size_t lo, hi;  // the clause's tokens [lo, hi)
    std::string err;
    int code = AQE_OK;

    int bad(size_t first, size_t last, const std::string& why, int rc = AQE_ERR_INVALID) {
        if (last >= hi) last = hi - 1;
        if (first > last) first = last;
        err = "key predicate '" + src.substr(tk[first].b, tk[last].e - tk[first].b) + "': " + why;
        code = rc;
        return rc;
    }

    // an int32 literal at token i
    int literal(size_t start, size_t i, int32_t* v) {
        if (i >= hi) return bad(start, hi - 1, "an integer literal is missing");
        const Tok& t = tk[i];
        if (t.kind == T_IDENT) return bad(start, i, "a key column is compared with int32 literals only, not with a column or an expression");
        if (t.kind != T_INT) return bad(start, i, "a key column is compared with int32 literals only (" + t.text + " is not an integer)");
        if (t.ival < std::numeric_limits<int32_t>::min() || t.ival > std::numeric_limits<int32_t>::max())
            return bad(start, i, t.text + " does not fit int32");
        *v = static_cast<int32_t>(t.ival);
        return AQE_OK;
    }

    // the term that starts at token i (a key column); *next: the token behind it
    int key_term(size_t i, aqe_key_filter* out, bool* seen, size_t* next) {
        const size_t start = i;
        const int col = key_column_of(tk[i]);
        aqe_key_term term;
        std::memset(&term, 0, sizeof term);
        ++i;
        bool negate = false;
        if (i < hi && is_word(tk[i], "NOT")) { negate = true; ++i; }
        if (i >= hi) return bad(start, hi - 1, "a comparison is missing");
        int rc = AQE_OK;
        if (tk[i].kind == T_OP && !negate) {
            const std::string op = tk[i].text;
            int32_t v = 0;
            rc = literal(start, i + 1, &v);
            if (rc != AQE_OK) return rc;
            const int32_t kMin = std::numeric_limits<int32_t>::min(), kMax = std::numeric_limits<int32_t>::max();
            if (op == "=") aqe_key_term_range(&term, v, v, 0);
            else if (op == "<>" || op == "!=") aqe_key_term_range(&term, v, v, 1);
            else if (op == ">=") aqe_key_term_range(&term, v, kMax, 0);
            else if (op == "<=") aqe_key_term_range(&term, kMin, v, 0);
            else if (op == ">") { if (v == kMax) aqe_key_term_range(&term, 1, 0, 0); else aqe_key_term_range(&term, v + 1, kMax, 0); }
            else if (op == "<") { if (v == kMin) aqe_key_term_range(&term, 1, 0, 0); else aqe_key_term_range(&term, kMin, v - 1, 0); }
            else return bad(start, i, "operator " + op + " is not one of = <> != >= > <= <");
            i += 2;
        } else if (is_word(tk[i], "IN")) {
            size_t j = i + 1;
            if (j >= hi || tk[j].kind != T_LP) return bad(start, j, "IN takes a parenthesised list of integers");
            ++j;
            std::vector<int32_t> vals;
            for (;;) {
                int32_t v = 0;
                rc = literal(start, j, &v);
                if (rc != AQE_OK) return rc;
                vals.push_back(v);
                ++j;
                if (j < hi && tk[j].kind == T_COMMA) { ++j; continue; }
                break;
            }
            if (j >= hi || tk[j].kind != T_RP) return bad(start, j, "IN list is not closed");
            rc = aqe_key_term_in(&term, vals.data(), static_cast<uint32_t>(vals.size()), negate ? 1 : 0);
            if (rc != AQE_OK)
                return bad(start, j, "the IN list spans more than " + std::to_string(AQE_KEY_BITMAP_BITS) + " consecutive key values", AQE_ERR_UNSUPPORTED);
            i = j + 1;
        } else if (is_word(tk[i], "BETWEEN")) {
            int32_t a = 0, b = 0;
            rc = literal(start, i + 1, &a);
            if (rc != AQE_OK) return rc;
            if (i + 2 >= hi || !is_word(tk[i + 2], "AND")) return bad(start, i + 2, "BETWEEN a AND b");
            rc = literal(start, i + 3, &b);
            if (rc != AQE_OK) return rc;
            if (a <= b) aqe_key_term_range(&term, a, b, negate ? 1 : 0);
            else aqe_key_term_range(&term, 1, 0, negate ? 1 : 0);  // BETWEEN 5 AND 3: no key
            i += 4;
        } else {
            return bad(start, i, "not one of =, <>, !=, >=, >, <=, <, [NOT] IN (...), [NOT] BETWEEN a AND b");
        }
        if (seen[col - 1]) return bad(start, i - 1, std::string("a second term on ") + (col == AQE_GROUP_REGION ? "region" : "product_id") + " (one term per key column)");
        seen[col - 1] = true;
        out->term[col - 1] = term;
        *next = i;
        return AQE_OK;
    }

    int run(aqe_key_filter* out) {
        bool seen[2] = {false, false};
        for (size_t i = lo; i < hi; ++i)
            if (is_word(tk[i], "OR")) return bad(lo, hi - 1, "OR is not supported beside a key predicate (a conjunction of terms only)");
        size_t i = lo;
        while (i < hi) {
            if (key_column_of(tk[i])) {
                int rc = key_term(i, out, seen, &i);
                if (rc != AQE_OK) return rc;
            } else {
                // a predicate on another column (the amount range): skipped, it is aqe_parse_where's; BETWEEN takes its own AND
                const size_t start = i;
                int depth = 0, between = 0;
                for (; i < hi; ++i) {
                    if (tk[i].kind == T_LP) ++depth;
                    else if (tk[i].kind == T_RP) --depth;
                    else if (is_word(tk[i], "BETWEEN")) ++between;
                    else if (is_word(tk[i], "AND") && depth <= 0) {
                        if (between > 0) --between;
                        else break;
                    } else if (key_column_of(tk[i])) {
                        return bad(start, i, "a key column may only stand on the left of a comparison with integer literals");
                    }
                }
            }
            if (i >= hi) break;
            if (!is_word(tk[i], "AND")) return bad(i, i, "AND expected between terms");
            ++i;
            if (i >= hi) return bad(i - 1, i - 1, "a term is missing after AND");
        }
        return AQE_OK;
    }
};

}  // namespace
}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_key_term_range(aqe_key_term* term, int32_t lo, int32_t hi, int negate) {
    if (!term) return AQE_ERR_INVALID;
    std::memset(term, 0, sizeof *term);
    term->form = AQE_KEYTERM_RANGE;
    term->negate = negate ? 1 : 0;
    term->lo = lo;
    term->hi = hi;
    return AQE_OK;
}

int aqe_key_term_in(aqe_key_term* term, const int32_t* values, uint32_t n, int negate) {
    if (!term || !values || n == 0) return AQE_ERR_INVALID;
    int32_t lo = values[0], hi = values[0];
    for (uint32_t i = 1; i < n; ++i) {
        lo = std::min(lo, values[i]);
        hi = std::max(hi, values[i]);
    }
    if (lo == hi) return aqe_key_term_range(term, lo, hi, negate);
    if (static_cast<int64_t>(hi) - lo >= AQE_KEY_BITMAP_BITS) return AQE_ERR_UNSUPPORTED;
    std::memset(term, 0, sizeof *term);
    term->form = AQE_KEYTERM_BITMAP;
    term->negate = negate ? 1 : 0;
    term->lo = lo;
    term->hi = hi;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t u = static_cast<uint32_t>(values[i]) - static_cast<uint32_t>(lo);
        term->bits[u >> 6] |= 1ull << (u & 63u);
    }
    return AQE_OK;
}

int aqe_parse_key_where(const char* query, aqe_key_filter* out, char* err, size_t err_cap) {
    if (err && err_cap) err[0] = '\0';
    if (!out) return AQE_ERR_INVALID;
    std::memset(out, 0, sizeof *out);
    const std::string src(query ? query : "");
    const std::vector<Tok> tk = tokenize(src);
    size_t lo = tk.size();
    for (size_t i = 0; i < tk.size(); ++i)
        if (is_word(tk[i], "WHERE")) { lo = i + 1; break; }
    size_t hi = lo;
    int depth = 0;
    for (; hi < tk.size(); ++hi) {
        const Tok& t = tk[hi];
        if (t.kind == T_LP) ++depth;
        else if (t.kind == T_RP) { if (--depth < 0) break; }
        else if (is_word(t, "GROUP") || is_word(t, "ORDER") || is_word(t, "LIMIT") || is_word(t, "HAVING") || (t.kind == T_OTHER && t.text == ";")) break;
    }
    bool named = false;
    for (size_t i = lo; i < hi; ++i) named = named || key_column_of(tk[i]) != 0;
    if (!named) return 0;
    KeyParse p{src, tk, lo, hi};
    const int rc = p.run(out);
    if (rc != AQE_OK) {
        std::memset(out, 0, sizeof *out);
        if (err && err_cap) std::snprintf(err, err_cap, "%s", p.err.c_str());
        return rc;
    }
    return 1;
}

int aqe_key_filter_test(const aqe_key_filter* filter, int32_t region, int32_t product_id) {
    if (!filter) return 0;
    const int32_t key[2] = {region, product_id};
    for (int k = 0; k < 2; ++k) {
        if (term_defect(filter->term[k])) return 0;
        DevTerm t;
        unsigned long long map[kMapWords];
        compile_term(filter->term[k], &t, map);
        if (!term_pass(t, map, key[k])) return 0;
    }
    return 1;
}

}  // extern "C"
