// fid_stag_layout.hip -- stag_ros::loadTagsBundles (stag_ros/load_yaml_tags.h:11-105) from the YAML file a deployer would hand to
// `rosparam load`: the `tags:` and `bundles:` parameters.  Part of the fid_api.hip translation unit; host code, no device.
//
// The reference reads XmlRpc values the parameter server made of the YAML; here the file itself is read.  Only the subset those two
// parameters need is parsed: block mappings and sequences by indentation, flow sequences / mappings ([..], {..}, over several lines
// too), plain and quoted scalars, comments, `---`.  No anchors, tags, multi-line scalars or multiple documents.
//   tags:    [{id, frame, corners: [[x, y, z] x 3]}, ...]                 parseTags     (:11-36)
//   bundles: [{frame, tags: [{id, corners: [[x, y, z] x 3]}, ...]}, ...]  parseBundles  (:38-73)
#include <stdio.h>

#include <stdexcept>

namespace {

thread_local std::string g_layout_error;

struct YNode {
    enum Kind { NUL, SCALAR, SEQ, MAP } kind = NUL;
    std::string scalar;
    std::vector<YNode> seq;
    std::vector<std::pair<std::string, YNode>> map;
    int line = 0;
    const YNode *get(const char *key) const
    {
        for (const auto &kv : map)
            if (kv.first == key) return &kv.second;
        return nullptr;
    }
};

struct YLine {
    int indent, no;
    std::string text;
};

struct YError : std::runtime_error {
    YError(int line, const std::string &what) : std::runtime_error("line " + std::to_string(line) + ": " + what) {}
};

std::string y_trim(const std::string &s)
{
    size_t a = 0, b = s.size();
    while (a < b && (s[a] == ' ' || s[a] == '\t' || s[a] == '\r')) a++;
    while (b > a && (s[b - 1] == ' ' || s[b - 1] == '\t' || s[b - 1] == '\r')) b--;
    return s.substr(a, b - a);
}

std::string y_unquote(const std::string &s)
{
    if (s.size() >= 2 && ((s.front() == '"' && s.back() == '"') || (s.front() == '\'' && s.back() == '\''))) return s.substr(1, s.size() - 2);
    return s;
}

// the text of a file as lines without comments and blanks
std::vector<YLine> y_lines(const std::string &text)
{
    std::vector<YLine> out;
    size_t pos = 0;
    int no = 0;
    while (pos <= text.size()) {
        size_t e = text.find('\n', pos);
        if (e == std::string::npos) e = text.size();
        std::string ln = text.substr(pos, e - pos);
        pos = e + 1;
        no++;
        char quote = 0;
        for (size_t i = 0; i < ln.size(); i++) {
            const char ch = ln[i];
            if (quote) {
                if (ch == quote) quote = 0;
            } else if (ch == '"' || ch == '\'') {
                quote = ch;
            } else if (ch == '#' && (i == 0 || ln[i - 1] == ' ' || ln[i - 1] == '\t')) {
                ln.erase(i);
                break;
            }
        }
        int indent = 0;
        while ((size_t)indent < ln.size() && ln[(size_t)indent] == ' ') indent++;
        if ((size_t)indent < ln.size() && ln[(size_t)indent] == '\t') throw YError(no, "tab in the indentation");
        const std::string t = y_trim(ln);
        if (t.empty() || t == "---" || t == "...") continue;
        out.push_back({indent, no, t});
    }
    return out;
}

// position of the ':' that ends a mapping key in `s` (followed by a space or the end; outside quotes and brackets), or npos
size_t y_key_colon(const std::string &s)
{
    char quote = 0;
    int depth = 0;
    for (size_t i = 0; i < s.size(); i++) {
        const char ch = s[i];
        if (quote) {
            if (ch == quote) quote = 0;
        } else if (ch == '"' || ch == '\'') {
            quote = ch;
        } else if (ch == '[' || ch == '{') {
            depth++;
        } else if (ch == ']' || ch == '}') {
            depth--;
        } else if (ch == ':' && depth == 0 && (i + 1 == s.size() || s[i + 1] == ' ')) {
            return i;
        }
    }
    return std::string::npos;
}

struct YFlow {
    const std::string &s;
    size_t p;
    int line;
    void ws()
    {
        while (p < s.size() && (s[p] == ' ' || s[p] == '\t' || s[p] == '\n' || s[p] == '\r')) p++;
    }
    YNode value()
    {
        ws();
        YNode n;
        n.line = line;
        if (p >= s.size()) throw YError(line, "value missing");
        if (s[p] == '[') {
            n.kind = YNode::SEQ;
            p++;
            ws();
            if (p < s.size() && s[p] == ']') {
                p++;
                return n;
            }
            for (;;) {
                n.seq.push_back(value());
                ws();
                if (p >= s.size()) throw YError(line, "']' missing");
                if (s[p] == ',') {
                    p++;
                    ws();
                    if (p < s.size() && s[p] == ']') {  // (a trailing comma)
                        p++;
                        return n;
                    }
                    continue;
                }
                if (s[p] == ']') {
                    p++;
                    return n;
                }
                throw YError(line, "',' or ']' expected");
            }
        }
        if (s[p] == '{') {
            n.kind = YNode::MAP;
            p++;
            ws();
            if (p < s.size() && s[p] == '}') {
                p++;
                return n;
            }
            for (;;) {
                ws();
                const std::string key = y_unquote(y_trim(scalar_until(":")));
                if (p >= s.size() || s[p] != ':' || key.empty()) throw YError(line, "'key: value' expected inside {}");
                p++;
                n.map.push_back({key, value()});
                ws();
                if (p >= s.size()) throw YError(line, "'}' missing");
                if (s[p] == ',') {
                    p++;
                    ws();
                    if (p < s.size() && s[p] == '}') {
                        p++;
                        return n;
                    }
                    continue;
                }
                if (s[p] == '}') {
                    p++;
                    return n;
                }
                throw YError(line, "',' or '}' expected");
            }
        }
        n.kind = YNode::SCALAR;
        n.scalar = y_unquote(y_trim(scalar_until(",]}")));
        if (n.scalar.empty()) throw YError(line, "value missing");
        return n;
    }
    std::string scalar_until(const char *stops)
    {
        const size_t a = p;
        char quote = 0;
        while (p < s.size()) {
            const char ch = s[p];
            if (quote) {
                if (ch == quote) quote = 0;
            } else if (ch == '"' || ch == '\'') {
                quote = ch;
            } else if (strchr(stops, ch) || ch == '[' || ch == '{') {
                break;
            }
            p++;
        }
        return s.substr(a, p - a);
    }
};

struct YParser {
    std::vector<YLine> L;
    size_t i = 0;

    static int depth_of(const std::string &s)
    {
        int d = 0;
        char quote = 0;
        for (char ch : s) {
            if (quote) {
                if (ch == quote) quote = 0;
            } else if (ch == '"' || ch == '\'') {
                quote = ch;
            } else if (ch == '[' || ch == '{') {
                d++;
            } else if (ch == ']' || ch == '}') {
                d--;
            }
        }
        return d;
    }
    // a value that starts in `first` on line i (already consumed from the line's text) and, if it is a flow collection, runs on
    // over the following lines until its brackets close
    YNode inline_value(const std::string &first, int line_no)
    {
        if (first[0] == '[' || first[0] == '{') {
            std::string all = first;
            int d = depth_of(all);
            while (d > 0) {
                if (i >= L.size()) throw YError(line_no, "file ends inside [ ] or { }");
                all += "\n" + L[i].text;
                d = depth_of(all);
                i++;
            }
            YFlow f{all, 0, line_no};
            YNode n = f.value();
            f.ws();
            if (f.p != all.size()) throw YError(line_no, "text after the closing bracket");
            return n;
        }
        YNode n;
        n.kind = YNode::SCALAR;
        n.line = line_no;
        n.scalar = y_unquote(first);
        return n;
    }
    YNode block(int indent)
    {
        YNode n;
        if (i >= L.size()) return n;
        n.line = L[i].no;
        const std::string &t0 = L[i].text;
        if (t0[0] == '-' && (t0.size() == 1 || t0[1] == ' ')) {
            n.kind = YNode::SEQ;
            while (i < L.size() && L[i].indent == indent && L[i].text[0] == '-' && (L[i].text.size() == 1 || L[i].text[1] == ' ')) {
                const std::string rest = y_trim(L[i].text.substr(1));
                if (rest.empty()) {
                    const int no = L[i].no;
                    i++;
                    if (i < L.size() && L[i].indent > indent) n.seq.push_back(block(L[i].indent));
                    else throw YError(no, "empty list item");
                } else {
                    // the item's content stands where the dash was: as a line of its own, indented past the dash
                    const int inner = indent + 1 + (int)(L[i].text.size() - 1 - y_trim_left_len(L[i].text.substr(1)));
                    L[i].indent = inner;
                    L[i].text = rest;
                    n.seq.push_back(block(inner));
                }
            }
            if (i < L.size() && L[i].indent > indent) throw YError(L[i].no, "unexpected indentation");
            return n;
        }
        const size_t colon = (t0[0] == '[' || t0[0] == '{') ? std::string::npos : y_key_colon(t0);
        if (colon == std::string::npos) {
            const int no = L[i].no;
            const std::string first = L[i].text;
            i++;
            return inline_value(first, no);
        }
        n.kind = YNode::MAP;
        while (i < L.size() && L[i].indent == indent) {
            const std::string t = L[i].text;
            const int no = L[i].no;
            if (t[0] == '-' && (t.size() == 1 || t[1] == ' ')) break;
            const size_t c = y_key_colon(t);
            if (c == std::string::npos || c == 0) throw YError(no, "'key: value' expected");
            const std::string key = y_unquote(y_trim(t.substr(0, c)));
            const std::string rest = y_trim(t.substr(c + 1));
            i++;
            YNode v;
            v.line = no;
            if (!rest.empty()) {
                v = inline_value(rest, no);
            } else if (i < L.size() && L[i].indent > indent) {
                v = block(L[i].indent);
            } else if (i < L.size() && L[i].indent == indent && L[i].text[0] == '-' && (L[i].text.size() == 1 || L[i].text[1] == ' ')) {
                v = block(indent);  // (a list under a key may stand at the key's own indentation)
            }
            for (const auto &kv : n.map)
                if (kv.first == key) throw YError(no, "key '" + key + "' twice");
            n.map.push_back({key, v});
        }
        if (i < L.size() && L[i].indent > indent) throw YError(L[i].no, "unexpected indentation");
        return n;
    }
    static size_t y_trim_left_len(const std::string &s)
    {
        size_t a = 0;
        while (a < s.size() && s[a] == ' ') a++;
        return s.size() - a;
    }
};

double y_number(const YNode &n, const char *what)
{
    if (n.kind != YNode::SCALAR) throw YError(n.line, std::string(what) + ": a number expected");
    char *end = nullptr;
    const double v = strtod(n.scalar.c_str(), &end);
    if (end == n.scalar.c_str() || *end != 0 || !(v == v) || v - v != 0) throw YError(n.line, std::string(what) + ": '" + n.scalar + "' is not a number");
    return v;
}

int y_int(const YNode &n, const char *what)
{
    if (n.kind != YNode::SCALAR) throw YError(n.line, std::string(what) + ": an integer expected");
    char *end = nullptr;
    const long v = strtol(n.scalar.c_str(), &end, 10);
    if (end == n.scalar.c_str() || *end != 0 || v < 0 || v > 0x7fffffffL) throw YError(n.line, std::string(what) + ": '" + n.scalar + "' is not a marker id");
    return (int)v;
}

// one entry of `tags:` or of a bundle's `tags:` (load_yaml_tags.h:17-30, :51-64)
fid_stag_tag y_tag(const YNode &n, int bundle, bool need_frame, std::string *frame)
{
    if (n.kind != YNode::MAP) throw YError(n.line, "a tag must be a mapping {id, corners}");
    const YNode *id = n.get("id"), *corners = n.get("corners"), *fr = n.get("frame");
    if (!id) throw YError(n.line, "tag without 'id'");
    if (!corners) throw YError(n.line, "tag without 'corners'");
    if (need_frame) {
        if (!fr || fr->kind != YNode::SCALAR || fr->scalar.empty()) throw YError(n.line, "tag without 'frame'");
        *frame = fr->scalar;
    }
    if (corners->kind != YNode::SEQ || corners->seq.size() != 3) throw YError(corners->line, "'corners' must list three corners [x, y, z]");
    double c[3][3];
    for (int k = 0; k < 3; k++) {
        const YNode &p = corners->seq[(size_t)k];
        if (p.kind != YNode::SEQ || p.seq.size() != 3) throw YError(p.line ? p.line : corners->line, "a corner must be three numbers [x, y, z]");
        for (int a = 0; a < 3; a++) c[k][a] = y_number(p.seq[(size_t)a], "corner");
    }
    fid_stag_tag t;
    (void)fid_stag_tag_from_three_corners(y_int(*id, "id"), bundle, c[0], c[1], c[2], &t);
    return t;
}

fid_status layout_load_impl(const char *path, fid_stag_tag *tags, int32_t tag_cap, int32_t *n_tags, int32_t *n_bundles, uint8_t *standalone,
                            char *frames, int32_t bundle_cap)
{
    g_layout_error.clear();
    if (n_tags) *n_tags = 0;
    if (n_bundles) *n_bundles = 0;
    if (!path || !n_tags || !n_bundles || tag_cap < 0 || bundle_cap < 0 || (tag_cap > 0 && !tags)) {
        g_layout_error = "invalid argument";
        return FID_E_INVALID_ARG;
    }
    std::string text;
    {
        FILE *fh = fopen(path, "rb");
        if (!fh) {
            g_layout_error = std::string("cannot open ") + path;
            return FID_E_INVALID_ARG;
        }
        char buf[4096];
        size_t got;
        while ((got = fread(buf, 1, sizeof(buf), fh)) > 0) text.append(buf, got);
        fclose(fh);
    }
    std::vector<fid_stag_tag> T;
    std::vector<std::string> F;
    std::vector<uint8_t> S;
    try {
        YParser P;
        P.L = y_lines(text);
        if (P.L.empty()) throw YError(1, "empty file");
        if (P.L[0].indent != 0) throw YError(P.L[0].no, "unexpected indentation");
        const YNode root = P.block(0);
        if (P.i != P.L.size()) throw YError(P.L[P.i].no, "unexpected text");
        if (root.kind != YNode::MAP) throw YError(root.line, "top level must be a mapping with 'tags' and / or 'bundles'");
        const YNode *yt = root.get("tags"), *yb = root.get("bundles");
        if (!yt && !yb) throw YError(root.line, "neither 'tags' nor 'bundles'");
        if (yb) {
            if (yb->kind != YNode::SEQ) throw YError(yb->line, "'bundles' must be a list");
            for (const YNode &b : yb->seq) {
                if (b.kind != YNode::MAP) throw YError(b.line, "a bundle must be a mapping {frame, tags}");
                const YNode *fr = b.get("frame"), *bt = b.get("tags");
                if (!fr || fr->kind != YNode::SCALAR || fr->scalar.empty()) throw YError(b.line, "bundle without 'frame'");
                if (!bt || bt->kind != YNode::SEQ || bt->seq.empty()) throw YError(b.line, "bundle without 'tags'");
                for (const YNode &t : bt->seq) T.push_back(y_tag(t, (int)F.size(), false, nullptr));
                F.push_back(fr->scalar);
                S.push_back(0);
            }
        }
        if (yt) {
            if (yt->kind != YNode::SEQ) throw YError(yt->line, "'tags' must be a list");
            for (const YNode &t : yt->seq) {
                std::string frame;
                T.push_back(y_tag(t, (int)F.size(), true, &frame));
                F.push_back(frame);
                S.push_back(1);
            }
        }
        for (size_t a = 0; a < T.size(); a++)
            for (size_t b = a + 1; b < T.size(); b++)
                if (T[a].id == T[b].id) throw YError(0, "id " + std::to_string(T[a].id) + " listed twice");
        for (const std::string &f : F)
            if (f.size() >= FID_STAG_FRAME_LEN) throw YError(0, "frame name '" + f + "' longer than " + std::to_string(FID_STAG_FRAME_LEN - 1) + " bytes");
    } catch (const YError &e) {
        g_layout_error = std::string(path) + ": " + e.what();
        return FID_E_INVALID_ARG;
    }
    *n_tags = (int32_t)T.size();
    *n_bundles = (int32_t)F.size();
    if ((int32_t)T.size() > tag_cap || ((standalone || frames) && (int32_t)F.size() > bundle_cap)) {
        g_layout_error = "buffers too small: " + std::to_string(T.size()) + " tags, " + std::to_string(F.size()) + " bundles";
        return FID_E_CAPACITY;
    }
    for (size_t k = 0; k < T.size(); k++) tags[k] = T[k];
    for (size_t k = 0; k < F.size(); k++) {
        if (standalone) standalone[k] = S[k];
        if (frames) {
            memset(frames + k * FID_STAG_FRAME_LEN, 0, FID_STAG_FRAME_LEN);
            memcpy(frames + k * FID_STAG_FRAME_LEN, F[k].data(), F[k].size());
        }
    }
    return FID_OK;
}

}  // namespace

extern "C" {

fid_status fid_stag_tag_from_three_corners(int32_t id, int32_t bundle, const double c0[3], const double c1[3], const double c2[3], fid_stag_tag *out)
{
    if (!c0 || !c1 || !c2 || !out) return FID_E_INVALID_ARG;
    out->id = id;
    out->bundle = bundle;
    for (int a = 0; a < 3; a++) {
        out->corners[0][a] = c0[a];
        out->corners[1][a] = c1[a];
        out->corners[2][a] = c2[a];
        out->center[a] = (c2[a] + c0[a]) / 2;          // t.center = (t.corners[2] + t.corners[0]) / 2
        out->corners[3][a] = c0[a] + (c2[a] - c1[a]);  // the vector C1 -> C2 from C0
    }
    return FID_OK;
}

fid_status fid_stag_layout_load_file(const char *path, fid_stag_tag *tags, int32_t tag_cap, int32_t *n_tags, int32_t *n_bundles,
                                     uint8_t *standalone, char *frames, int32_t bundle_cap)
{
    try {
        return layout_load_impl(path, tags, tag_cap, n_tags, n_bundles, standalone, frames, bundle_cap);
    } catch (const std::bad_alloc &) {
        g_layout_error = "out of memory";
        return FID_E_OUT_OF_MEMORY;
    } catch (const std::exception &e) {
        g_layout_error = std::string("damaged file: ") + e.what();
        return FID_E_INVALID_ARG;
    }
}

const char *fid_stag_layout_last_error(void) { return g_layout_error.c_str(); }

}  // extern "C"
