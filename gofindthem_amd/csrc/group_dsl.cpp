// group_dsl.cpp -- see group_dsl.hpp
#include "group_dsl.hpp"

#include "dsl_compile.hpp"

namespace gft {
namespace gdsl {

const char* token_name(Token t) {
    static const char* n[] = {"ILLEGAL", "EOF", "WS", "TAG", "FIELD_PATH", "QUOTATION", "OPPAR", "CLPAR", "AND", "OR", "NOT"};
    return (int)t >= 0 && (int)t < 11 ? n[t] : "UNEXPECTED";
}
const char* expr_type_name(ExprType t) {
    static const char* n[] = {"UNSET", "AND", "OR", "NOT", "UNIT"};
    return (int)t >= 0 && (int)t < 5 ? n[t] : "UNEXPECTED";
}

namespace {
std::string rune_str(int32_t cp) { std::string s; dsl::EncodeRune(cp, s); return s; }
bool is_ws(int32_t c) { return c == ' ' || c == '\t' || c == '\n'; }
bool is_letter(int32_t c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }
std::string trim_spaces(const std::string& s) {          // strings.Trim(s, " ")
    size_t a = 0, b = s.size();
    while (a < b && s[a] == ' ') a++;
    while (b > a && s[b - 1] == ' ') b--;
    return s.substr(a, b - a);
}
}  // namespace

// ---- scanner (group/dsl/scanner.go) -----------------------------------------------------------------------
int32_t Scanner::read() {                 // rune 0 doubles as the end marker (scanner.go:263)
    if (i_ >= s_.size()) { last_ = 0; return 0; }
    size_t adv;
    const int32_t cp = dsl::DecodeRune(s_, i_, &adv);
    i_ += adv;
    last_ = adv;
    return cp;
}
void Scanner::unread() { i_ -= last_; last_ = 0; }

ScanResult Scanner::Scan() {              // scanner.go:78-109
    ScanResult r;
    const int32_t ch = read();
    if (is_ws(ch)) { unread(); return scan_whitespace(); }
    if (ch == '"') { unread(); return scan_tag(); }
    if (ch == ':') { unread(); return scan_field_path(); }
    if (is_letter(ch)) { unread(); return scan_operators(); }
    if (ch == '(') { r.tok = OPPAR; r.lit = "("; return r; }
    if (ch == ')') { r.tok = CLPAR; r.lit = ")"; return r; }
    if (ch == 0) { r.tok = END_OF_INPUT; return r; }
    r.err = "illegal char was found " + rune_str(ch);
    return r;
}

ScanResult Scanner::scan_whitespace() {   // scanner.go:112-131
    ScanResult r;
    dsl::EncodeRune(read(), r.lit);
    for (;;) {
        const int32_t ch = read();
        if (ch == 0) break;
        if (!is_ws(ch)) { unread(); break; }
        dsl::EncodeRune(ch, r.lit);
    }
    r.tok = WS;
    return r;
}

ScanResult Scanner::scan_operators() {    // scanner.go:134-172
    ScanResult r;
    int32_t ch = read();
    if (!is_letter(ch)) { r.err = "fail to scan operator: expected letter but found " + rune_str(ch); return r; }
    std::string lit(1, (char)ch);
    for (;;) {
        ch = read();
        if (ch == 0) break;
        if (!is_letter(ch)) { unread(); break; }
        lit.push_back((char)ch);
    }
    std::string up = lit;
    for (char& c : up) if (c >= 'a' && c <= 'z') c = (char)(c - 32);
    if (up == "AND") r.tok = AND;
    else if (up == "OR") r.tok = OR;
    else if (up == "NOT") r.tok = NOT;
    else { r.err = "failed to scan operator: unexpected operator '" + lit + "' found"; return r; }
    r.lit = lit;
    return r;
}

ScanResult Scanner::scan_tag() {          // scanner.go:177-210
    ScanResult r;
    int32_t ch = read();
    if (ch != '"') { r.err = "fail to scan tag: expected \" but found " + rune_str(ch); return r; }
    std::string buf;
    for (;;) {
        ch = read();
        if (ch == 0) { r.err = "fail to scan tag: expected ':' but found EOF"; return r; }
        if (ch == '\\') {
            const int32_t esc = read();
            if (esc == '\\' || esc == '"' || esc == ':') dsl::EncodeRune(esc, buf);
            else { r.err = "fail to scan tag: invalid escaped char " + rune_str(esc); return r; }
            continue;
        }
        if (ch == ':') { unread(); break; }      // the field path is the next token
        if (ch == '"') break;
        dsl::EncodeRune(ch, buf);
    }
    r.lit = trim_spaces(buf);
    r.tok = TAG;
    return r;
}

ScanResult Scanner::scan_field_path() {   // scanner.go:215-244
    ScanResult r;
    int32_t ch = read();
    if (ch != ':') { r.err = "fail to scan field: expected ':' but found " + rune_str(ch); return r; }
    std::string buf;
    for (;;) {
        ch = read();
        if (ch == 0) { r.err = "fail to scan field: expected '\"' but found EOF"; return r; }
        if (ch == '\\') {
            const int32_t esc = read();
            if (esc == '\\' || esc == '"') dsl::EncodeRune(esc, buf);
            else { r.err = "fail to scan field: invalid escaped char " + rune_str(esc); return r; }
            continue;
        }
        if (ch == '"') break;
        dsl::EncodeRune(ch, buf);
    }
    r.lit = trim_spaces(buf);
    r.tok = FIELD_PATH;
    return r;
}

// ---- parser (group/dsl/parser.go) --------------------------------------------------------------------------
namespace {

struct Parser {
    Scanner s;
    struct { Token tok = ILLEGAL; std::string lit; bool unscanned = false; } buf;
    int parCount = 0;
    std::vector<std::string> tags, fields;

    explicit Parser(const std::string& src) : s(src) {}

    static void add_unique(std::vector<std::string>& v, const std::string& x) {
        for (const auto& y : v) if (y == x) return;
        v.push_back(x);
    }

    ScanResult scan() {                                   // parser.go:204-219
        if (buf.unscanned) { buf.unscanned = false; ScanResult r; r.tok = buf.tok; r.lit = buf.lit; return r; }
        ScanResult r = s.Scan();
        if (!r.err.empty()) return r;
        buf.tok = r.tok; buf.lit = r.lit;
        return r;
    }
    void unscan() { buf.unscanned = true; }
    ScanResult scan_ignore_ws() {                         // parser.go:226-235
        ScanResult r = scan();
        if (!r.err.empty()) return r;
        if (r.tok == WS) r = scan();
        return r;
    }

    std::string parse_tag_info(TagInfo& tag) {            // parser.go:252-278
        ScanResult r = scan_ignore_ws();
        if (!r.err.empty()) return r.err;
        if (r.tok != TAG) return std::string("invalid expression: Expecting TAG but found ") + token_name(r.tok);
        if (r.lit.empty()) return "invalid expression: Found empty TAG";
        tag.Name = r.lit;
        ScanResult n = scan_ignore_ws();
        if (!n.err.empty()) return n.err;
        if (n.tok != FIELD_PATH) { unscan(); return ""; }
        tag.FieldPath = n.lit;
        return "";
    }

    void note(const TagInfo& tag) {
        add_unique(tags, tag.Name);
        if (!tag.FieldPath.empty()) add_unique(fields, tag.FieldPath);
    }

    std::string handle_open_par(std::unique_ptr<Expression>& out) {   // parser.go:238-249
        const int parlvl = parCount;
        parCount++;
        std::string err = parse(out);
        if (!err.empty()) return err;
        if (parCount != parlvl) return "invalid expression: Unexpected '('";
        return "";
    }

    // parser.go:178-201; exp is replaced by the node the caller continues with
    std::string handle_dual_op(std::unique_ptr<Expression>& exp, ExprType type) {
        if (!exp->LExpr) return std::string("invalid expression: no left expression was found for ") + expr_type_name(type);
        if (!exp->RExpr) { exp->Type = type; return ""; }
        std::unique_ptr<Expression> up(new Expression());
        up->Type = type;
        up->LExpr = std::move(exp);
        exp = std::move(up);
        ScanResult n = scan_ignore_ws();
        if (!n.err.empty()) return n.err;
        if (n.tok == OPPAR) {
            std::unique_ptr<Expression> sub;
            std::string err = handle_open_par(sub);
            if (!err.empty()) return err;
            exp->RExpr = std::move(sub);
        } else {
            unscan();
        }
        return "";
    }

    static void attach(Expression& exp, std::unique_ptr<Expression> child) {
        if (!exp.LExpr) exp.LExpr = std::move(child); else exp.RExpr = std::move(child);
    }

    std::string parse(std::unique_ptr<Expression>& out) {  // parser.go:41-175
        std::unique_ptr<Expression> exp(new Expression());
        for (;;) {
            ScanResult r = scan_ignore_ws();
            if (!r.err.empty()) return r.err;
            switch (r.tok) {
            case OPPAR: {
                std::unique_ptr<Expression> sub;
                std::string err = handle_open_par(sub);
                if (!err.empty()) return err;
                attach(*exp, std::move(sub));
                break;
            }
            case TAG: {
                unscan();
                TagInfo tag;
                std::string err = parse_tag_info(tag);
                if (!err.empty()) return err;
                std::unique_ptr<Expression> unit(new Expression());
                unit->Type = UNIT_EXPR;
                unit->Tag = tag;
                attach(*exp, std::move(unit));
                note(tag);
                break;
            }
            case AND:
            case OR: {
                std::string err = handle_dual_op(exp, r.tok == AND ? AND_EXPR : OR_EXPR);
                if (!err.empty()) return err;
                break;
            }
            case NOT: {
                ScanResult n = scan_ignore_ws();
                if (!n.err.empty()) return n.err;
                std::unique_ptr<Expression> neg(new Expression());
                neg->Type = NOT_EXPR;
                if (n.tok == TAG) {
                    unscan();
                    TagInfo tag;
                    std::string err = parse_tag_info(tag);
                    if (!err.empty()) return err;
                    neg->RExpr.reset(new Expression());
                    neg->RExpr->Type = UNIT_EXPR;
                    neg->RExpr->Tag = tag;
                    note(tag);
                } else if (n.tok == OPPAR) {
                    std::unique_ptr<Expression> sub;
                    std::string err = handle_open_par(sub);
                    if (!err.empty()) return err;
                    neg->RExpr = std::move(sub);
                } else {
                    return std::string("invalid expression: Unexpected token '") + token_name(n.tok) + "' after NOT";
                }
                attach(*exp, std::move(neg));
                break;
            }
            case CLPAR:
                parCount--;
                // fall through
            case END_OF_INPUT: {
                if (parCount < 0)
                    return "invalid expression: unexpected EOF found. Extra closing parentheses: " + std::to_string(-parCount);
                std::unique_ptr<Expression> fin;
                if (exp->Type == UNSET_EXPR) {
                    if (exp->RExpr) fin = std::move(exp->RExpr);
                    else if (exp->LExpr) fin = std::move(exp->LExpr);
                    else return "invalid expression: unexpected EOF found";
                } else {
                    fin = std::move(exp);
                }
                if ((fin->Type == AND_EXPR || fin->Type == OR_EXPR) && !fin->RExpr)
                    return std::string("invalid expression: incomplete expression ") + expr_type_name(fin->Type);
                out = std::move(fin);
                return "";
            }
            default:
                return "invalid expression: Unexpected operator was found (" + std::to_string((int)r.tok) + " = '" + r.lit + "')";
            }
        }
    }
};

}  // namespace

ParseResult Parse(const std::string& src) {
    ParseResult res;
    Parser p(src);
    res.err = p.parse(res.expr);
    if (!res.err.empty()) res.expr.reset();
    res.tags = p.tags;
    res.fields = p.fields;
    return res;
}

bool Solve(const Expression& e, const TagMap& m, std::string& err) {
    return SolveWith(e, [&](const Expression& u) {
        auto it = m.find(u.Tag.Name);
        if (it == m.end()) return false;
        if (u.Tag.FieldPath.empty()) return true;
        for (const auto& fp : it->second)
            if (fp.first.compare(0, u.Tag.FieldPath.size(), u.Tag.FieldPath) == 0) return true;
        return false;
    }, err);
}

std::string ToJson(const Expression& e) {
    std::string o = "{\"Type\":\"";
    o += expr_type_name(e.Type);
    o += "\"";
    if (e.Type == UNIT_EXPR) {
        o += ",\"Tag\":{\"Name\":";
        dsl::json_str(e.Tag.Name, o);
        o += ",\"FieldPath\":";
        dsl::json_str(e.Tag.FieldPath, o);
        o += "}";
    }
    if (e.LExpr) { o += ",\"LExpr\":"; o += ToJson(*e.LExpr); }
    if (e.RExpr) { o += ",\"RExpr\":"; o += ToJson(*e.RExpr); }
    o += "}";
    return o;
}

}  // namespace gdsl

// ---- what the finder asks of a field path (group/finder/internal.go) ----------------------------------------------------------
bool IsValidFieldPath(const std::string& fieldPath, const std::vector<std::string>& includePaths,
                      const std::vector<std::string>& excludePaths) {
    for (const auto& x : excludePaths)
        if (fieldPath.compare(0, x.size(), x) == 0) return false;
    if (!includePaths.empty()) {
        for (const auto& x : includePaths)
            if (fieldPath.compare(0, x.size(), x) == 0) return true;
        return false;
    }
    return true;
}

}  // namespace gft
