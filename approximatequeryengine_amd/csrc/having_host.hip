// having_host.hip — the host-only side of HAVING on grouped aggregates (contract in include/aqe_hip.h): the clause's grammar
// (aqe_parse_having), one term against one figure (aqe_having_test) and the judging over a vector of bins
// (aqe_having_from_bins).  No GPU and no context; the semantics are having_core.hpp's, the copy the kernels of wide_group.hip
// compile, so bins judged here and there give the same groups, counters and bytes.
#include <cctype>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "having_core.hpp"
#include "host.hpp"

namespace aqe {
namespace {

struct Tok {
    enum Kind { kEnd, kWord, kNumber, kSym } kind;
    std::string text;  // a word in upper case; a symbol as written
    double num;
};

bool word_at(const std::string& up, size_t i, const char* w) {
    const size_t n = std::strlen(w);
    if (up.compare(i, n, w) != 0) return false;
    const auto is_id = [](char ch) { return std::isalnum(static_cast<unsigned char>(ch)) || ch == '_'; };
    return (i == 0 || !is_id(up[i - 1])) && (i + n >= up.size() || !is_id(up[i + n]));
}

// The clause of `text`: what follows the word HAVING (the whole text without one), up to ORDER BY, LIMIT, ';' or " --".
std::string clause_of(const char* text) {
    std::string s(text), up(s);
    for (char& ch : up) ch = static_cast<char>(std::toupper(static_cast<unsigned char>(ch)));
    size_t lo = 0;
    for (size_t i = 0; i + 6 <= up.size(); ++i)
        if (word_at(up, i, "HAVING")) { lo = i + 6; break; }
    size_t hi = s.size();
    for (size_t i = lo; i < hi; ++i) {
        if (s[i] == ';' || word_at(up, i, "LIMIT") || word_at(up, i, "ORDER")) { hi = i; break; }
        if (s[i] == '-' && i + 1 < s.size() && s[i + 1] == '-' && (i == lo || std::isspace(static_cast<unsigned char>(s[i - 1])))) { hi = i; break; }
    }
    return s.substr(lo, hi - lo);
}

std::vector<Tok> lex(const std::string& s) {
    std::vector<Tok> out;
    size_t i = 0;
    while (i < s.size()) {
        const unsigned char ch = static_cast<unsigned char>(s[i]);
        if (std::isspace(ch)) { ++i; continue; }
        if (std::isalpha(ch) || ch == '_') {
            size_t j = i;
            std::string w;
            while (j < s.size() && (std::isalnum(static_cast<unsigned char>(s[j])) || s[j] == '_')) w += static_cast<char>(std::toupper(static_cast<unsigned char>(s[j++])));
            out.push_back(Tok{Tok::kWord, w, 0.0});
            i = j;
        } else if (std::isdigit(ch) || (ch == '.' && i + 1 < s.size() && std::isdigit(static_cast<unsigned char>(s[i + 1])))) {
            char* end = nullptr;
            const double v = std::strtod(s.c_str() + i, &end);
            const size_t j = static_cast<size_t>(end - s.c_str());
            out.push_back(Tok{Tok::kNumber, s.substr(i, j - i), v});
            i = j;
        } else {
            std::string sym(1, s[i]);
            if (i + 1 < s.size() && ((s[i] == '>' && s[i + 1] == '=') || (s[i] == '<' && (s[i + 1] == '=' || s[i + 1] == '>')) || (s[i] == '!' && s[i + 1] == '=')))
                sym += s[i + 1];
            out.push_back(Tok{Tok::kSym, sym, 0.0});
            i += sym.size();
        }
    }
    out.push_back(Tok{Tok::kEnd, "the end of the clause", 0.0});
    return out;
}

struct Parser {
    std::vector<Tok> t;
    size_t at = 0;
    std::string why;

    const Tok& peek() const { return t[at]; }
    bool is_word(const char* w) const { return peek().kind == Tok::kWord && peek().text == w; }
    bool is_sym(const char* s) const { return peek().kind == Tok::kSym && peek().text == s; }
    bool no(const std::string& msg) { if (why.empty()) why = msg; return false; }

    bool number(double* v) {
        double sign = 1.0;
        if (is_sym("-") || is_sym("+")) { sign = is_sym("-") ? -1.0 : 1.0; ++at; }
        if (is_word("INF") || is_word("INFINITY") || is_word("NAN")) return no("a threshold is not a finite number ('" + peek().text + "')");
        if (peek().kind != Tok::kNumber) return no("a number is expected, found '" + peek().text + "'");
        *v = sign * peek().num;
        if (*v - *v != 0.0) return no("a threshold is not a finite number ('" + peek().text + "')");
        ++at;
        if (is_sym("+") || is_sym("-") || is_sym("*") || is_sym("/") || is_sym("%"))
            return no("arithmetic is not supported: a threshold is one number, found '" + peek().text + "' behind it");
        return true;
    }

    bool term(aqe_having_term* out) {
        if (peek().kind != Tok::kWord) return no("a term begins with SUM, AVG or COUNT, found '" + peek().text + "'");
        const std::string name = peek().text;
        ++at;
        if (!is_sym("(")) return no("a term begins with SUM(amount), AVG(amount) or COUNT(*): '" + name + "' is not one of them, and an alias is not resolved");
        if (name == "SUM") out->agg = AQE_SUM;
        else if (name == "AVG") out->agg = AQE_AVG;
        else if (name == "COUNT") out->agg = AQE_COUNT;
        else return no("HAVING judges SUM, AVG or COUNT, not " + name);
        ++at;
        if (is_sym("*")) {
            if (out->agg != AQE_COUNT) return no("* is only for COUNT: " + name + "(amount)");
        } else if (!is_word("AMOUNT")) {
            return no("the aggregate of a term is over amount (or COUNT(*)), found '" + peek().text + "'");
        }
        ++at;
        if (!is_sym(")")) return no("')' is expected behind the aggregate's column (arithmetic is not supported), found '" + peek().text + "'");
        ++at;
        out->b = 0.0;
        bool between = false;
        if (is_sym(">")) out->op = AQE_HAVING_GT;
        else if (is_sym(">=")) out->op = AQE_HAVING_GE;
        else if (is_sym("<")) out->op = AQE_HAVING_LT;
        else if (is_sym("<=")) out->op = AQE_HAVING_LE;
        else if (is_sym("=")) return no("= is refused: equality on an estimate is meaningless (use BETWEEN)");
        else if (is_sym("<>") || is_sym("!=")) return no("<> is refused: inequality on an estimate is meaningless (use NOT BETWEEN)");
        else if (is_word("BETWEEN")) { out->op = AQE_HAVING_BETWEEN; between = true; }
        else if (is_word("NOT")) {
            ++at;
            if (!is_word("BETWEEN")) return no("NOT is followed by BETWEEN, found '" + peek().text + "'");
            out->op = AQE_HAVING_NOT_BETWEEN;
            between = true;
        } else if (is_sym("+") || is_sym("-") || is_sym("*") || is_sym("/") || is_sym("%")) {
            return no("arithmetic is not supported: an operator (>, >=, <, <=, BETWEEN, NOT BETWEEN) follows the aggregate, found '" + peek().text + "'");
        } else {
            return no("an operator (>, >=, <, <=, BETWEEN, NOT BETWEEN) is expected, found '" + peek().text + "'");
        }
        ++at;
        if (!number(&out->a)) return false;
        if (between) {
            if (!is_word("AND")) return no("BETWEEN x AND y: AND is expected, found '" + peek().text + "'");
            ++at;
            if (!number(&out->b)) return false;
            if (out->a > out->b) return no("BETWEEN x AND y takes x <= y");
        }
        return true;
    }

    bool condition(aqe_having_spec* out) {
        std::memset(out, 0, sizeof *out);
        for (;;) {
            if (out->nterms == AQE_HAVING_MAX_TERMS) return no("a third term: a condition is at most 2 terms joined by AND");
            if (!term(&out->term[out->nterms])) return false;
            ++out->nterms;
            if (peek().kind == Tok::kEnd) return true;
            if (is_word("OR")) return no("OR is not supported: a condition is terms joined by AND");
            if (!is_word("AND")) return no("AND or the end of the clause is expected, found '" + peek().text + "'");
            ++at;
        }
    }
};

}  // namespace
}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_parse_having(const char* text, aqe_having_spec* out) {
    if (!text || !out) return fail(nullptr, AQE_ERR_INVALID, "null argument");
    Parser p;
    p.t = lex(clause_of(text));
    if (!p.condition(out)) {
        std::memset(out, 0, sizeof *out);
        return fail(nullptr, AQE_ERR_INVALID, "HAVING: " + p.why);
    }
    return AQE_OK;
}

int aqe_having_test(const aqe_having_term* term, double value, double ci_lower, double ci_upper, int* passes, int* settled) {
    if (!term || !passes || !settled) return fail(nullptr, AQE_ERR_INVALID, "null argument");
    aqe_having_spec one{};
    one.nterms = 1;
    one.term[0] = *term;
    if (const char* why = having_spec_error(one)) return fail(nullptr, AQE_ERR_INVALID, std::string("HAVING: ") + why);
    bool p = false, s = false;
    having_term_test(*term, value, ci_lower, ci_upper, p, s);
    *passes = p ? 1 : 0;
    *settled = s ? 1 : 0;
    return AQE_OK;
}

int aqe_having_from_bins(const double* bins, uint32_t nbins, int ncols, const int32_t* key_min, const uint32_t* span, double shift, const aqe_query* q,
                         const aqe_having_spec* having, aqe_group_result* out, uint32_t cap, uint32_t* n_listed, aqe_having_info* info) {
    if (!q || !having || !n_listed || !info || !key_min || !span || (nbins && !bins) || (cap && !out)) return fail(nullptr, AQE_ERR_INVALID, "null argument");
    *n_listed = 0;
    std::memset(info, 0, sizeof *info);
    if (const char* why = having_spec_error(*having)) return fail(nullptr, AQE_ERR_INVALID, std::string("HAVING: ") + why);
    if (q->agg != AQE_SUM && q->agg != AQE_AVG && q->agg != AQE_COUNT) return fail(nullptr, AQE_ERR_INVALID, "GROUP BY (wide) takes SUM, AVG or COUNT");
    if (!(q->sample_percent > 0.0)) return fail(nullptr, AQE_ERR_INVALID, "sample_percent must be positive");
    if (ncols != 1 && ncols != 2) return fail(nullptr, AQE_ERR_INVALID, "GROUP BY (wide): one group column or a pair of them");
    const uint64_t want = ncols == 2 ? static_cast<uint64_t>(span[0]) * span[1] : span[0];
    if (want != nbins || nbins > 65536u) return fail(nullptr, AQE_ERR_INVALID, "HAVING: the spans do not give " + std::to_string(nbins) + " bins (at most 65536)");
    const PairRange g{key_min[0], ncols == 2 ? key_min[1] : 0, span[0], ncols == 2 ? span[1] : 1u};
    double c = shift;  // (query_shift's clamp into the amount range)
    if (q->has_where && q->where_min <= q->where_max) c = std::min(std::max(c, q->where_min), q->where_max);
    uint32_t count = 0;
    for (uint32_t b = 0; b < nbins; ++b) {
        const double* const v = bins + static_cast<size_t>(b) * 4;
        const unsigned m = having_mark(*having, v[0], v[1], v[2], v[3], c, q->sample_percent);
        info->groups += mark_group(m);
        info->candidates += mark_candidate(m);
        info->passed += mark_passed(m);
        info->passed_unsettled += mark_passed_unsettled(m);
        info->failed_unsettled += mark_failed_unsettled(m);
        if (!mark_passed(m)) continue;
        if (count < cap) {
            const int64_t key = ncols == 2 ? pair_key(g, b) : static_cast<int64_t>(g.kmin_a) + b;
            out[count] = wide_result(v[0], v[1], v[2], v[3], key, c, q->sample_percent, q->agg);
        }
        ++count;
    }
    *n_listed = count;
    if (count > cap && cap) std::memset(out, 0, sizeof(aqe_group_result) * cap);  // no partial list
    if (count > cap) return fail(nullptr, AQE_ERR_INVALID, "HAVING: " + std::to_string(count) + " groups pass, more than the caller's buffer holds (cap " + std::to_string(cap) + ")");
    return AQE_OK;
}

}  // extern "C"
