// jplace output of the placements on a fixed backbone (`-o j`; no reference counterpart).  Format: Matsen et al. 2012, "A format
// for phylogenetic placements", version 3 -- what pplacer, EPA-ng and APPLES write and gappa, guppy and iTOL read.
#include "dipper_host.hpp"

#include <cmath>
#include <cstdio>

namespace dipper {

// a JSON string literal
static void putJson(TextBuf& out, const std::string& v)
{
    out.put('"');
    for (unsigned char ch : v) {
        if (ch == '"' || ch == '\\') { out.put('\\'); out.put((char)ch); }
        else if (ch < 0x20) { char b[8]; std::snprintf(b, sizeof b, "\\u%04x", ch); out.put(b); }
        else out.put((char)ch);
    }
    out.put('"');
}

// JSON has no token for a NaN or an infinity (`%.17g` would print the bare words nan / inf, which no reader of jplace accepts):
// placeFixed hands over finite rows only, and a caller that does not is refused before a byte of the file is written
static void putDouble(TextBuf& out, double v)
{
    if (!std::isfinite(v)) die("ERROR: jplace: a placement with a length that is not finite cannot be written");
    char b[40];
    std::snprintf(b, sizeof b, "%.17g", v);
    out.put(b);
}

// the backbone as the -t file has it: children in file order, a non-root node followed by `:length{k}`, k = its place in
// post-order among the non-root nodes -- the edge numbering of KPlacementDeviceArrays::initializeDeviceArrays
static std::string jplaceTree(const Tree& t)
{
    TextBuf out;
    out.s.reserve(t.nodes.size() * 32);
    struct Frame { int node; size_t next; };
    std::vector<Frame> st;
    st.push_back(Frame{ t.root, 0 });
    size_t edge = 0;
    while (!st.empty()) {
        Frame& f = st.back();
        const Node& nd = t.nodes[(size_t)f.node];
        if (f.next == 0) { if (nd.children.empty()) out.put(nd.name); else out.put('('); }
        if (f.next < nd.children.size()) {
            if (f.next > 0) out.put(',');
            const int c = nd.children[f.next++];
            st.push_back(Frame{ c, 0 });
            continue;
        }
        if (!nd.children.empty()) out.put(')');
        if (nd.parent >= 0) {
            out.put(':'); out.putLength(nd.bl);
            out.put('{'); out.put(std::to_string(edge++)); out.put('}');
        }
        st.pop_back();
    }
    out.put(';');
    return out.s;
}

static const char* distanceName(const Param& params)
{
    if (params.in == "r") return "mash";
    switch (params.distanceType) {
    case DPR_DIST_UNCORRECTED: return params.protein ? "protein uncorrected" : "uncorrected";
    case DPR_DIST_JC: return params.protein ? "protein JC (20 states)" : "JC";
    case DPR_DIST_POISSON: return "protein Poisson";
    case DPR_DIST_KIMURA: return "protein Kimura";
    case DPR_DIST_TAJIMANEI: return "Tajima-Nei";
    case DPR_DIST_K2P: return "K2P";
    case DPR_DIST_TAMURA: return "Tamura";
    case DPR_DIST_JINNEI: return "Jinnei";
    case DPR_DIST_TN93: return "TN93";
    case DPR_DIST_LOGDET: return "LogDet";
    case DPR_DIST_PARALINEAR: return "paralinear";
    }
    return "unknown";
}

void writeJplace(std::ostream& os, const Tree& t, const std::vector<std::string>& names, const std::vector<std::vector<PlacementRow>>& rows,
                 const Param& params, const BootstrapOptions& bo)
{
    TextBuf out;
    out.s.reserve(rows.size() * 96 + t.nodes.size() * 40);
    out.put("{\n\"version\":3,\n\"tree\":");
    putJson(out, jplaceTree(t));
    out.put(",\n\"fields\":[\"edge_num\",\"likelihood\",\"like_weight_ratio\",\"distal_length\",\"pendant_length\"],\n\"placements\":[");
    const size_t backbone = t.m_numLeaves;
    bool first = true;
    for (size_t q = 0; q < rows.size(); ++q) {
        if (rows[q].empty()) continue;      // (a query without a finite placement: placeFixed)
        out.put(first ? "\n{\"p\":[" : ",\n{\"p\":[");
        first = false;
        for (size_t k = 0; k < rows[q].size(); ++k) {
            const PlacementRow& r = rows[q][k];
            if (k) out.put(',');
            out.put('['); out.put(std::to_string(r.edge)); out.put(",0,");
            putDouble(out, bo.replicates > 0 ? (double)r.count / (double)bo.replicates : 1.0); out.put(',');
            putDouble(out, r.distal); out.put(',');
            putDouble(out, r.pendant); out.put(']');
        }
        out.put("],\"n\":["); putJson(out, names[backbone + q]); out.put("]}");
    }
    out.put("\n],\n\"metadata\":{\"software\":\"dipper\",\"placement\":\"k-closest distance placement on a fixed backbone\",\"distance\":");
    putJson(out, distanceName(params));
    if (params.in == "r") { out.put(",\"kmer_size\":"); out.put(std::to_string(params.kmerSize)); out.put(",\"sketch_size\":"); out.put(std::to_string(params.sketchSize)); }
    if (bo.replicates > 0) {
        out.put(",\"bootstrap_replicates\":"); out.put(std::to_string(bo.replicates));
        out.put(",\"bootstrap_seed\":"); out.put(std::to_string(bo.seed));
    }
    if (!params.siteCoverage.empty()) {
        out.put(",\"site_coverage\":"); putJson(out, params.siteCoverage);
        out.put(",\"sites_kept\":"); out.put(std::to_string(params.sitesKept));
    }
    out.put("}\n}\n");
    os.write(out.s.data(), (std::streamsize)out.s.size());
}

}  // namespace dipper
