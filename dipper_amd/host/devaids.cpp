// dipper -- the six --dump-* developer aids of the command line (no GPU): the host-side readers, packers and writers run on
// their own, for the tests that compare them with the reference's and under the sanitizers (make asan).
#include "options.hpp"

#include <algorithm>
#include <fstream>
#include <iostream>

namespace dipper {

int runDeveloperAid(const Options& o)
{
    if (o.aid == "dump-tree") {
        // developer aid (no GPU): parse --input-tree with totalLeaves = arg and print the node table
        std::ifstream tf(o.treeFile);
        if (!tf) { std::cerr << "ERROR: Unable to open input tree file: " << o.treeFile << "\n"; return 1; }
        std::string nwk;
        std::getline(tf, nwk);
        size_t totalLeaves = 0;
        try { totalLeaves = (size_t)std::stoi(o.aidArg); } catch (...) {}
        Tree t(nwk, totalLeaves);
        std::printf("%zu %zu %d\n", t.nodes.size(), t.m_numLeaves, t.nodes[(size_t)t.root].idx);
        for (const Node& nd : t.nodes)
            std::printf("%d %d %.17g %d %s\n", nd.idx, nd.parent >= 0 ? t.nodes[(size_t)nd.parent].idx : -1, nd.bl,
                        nd.children.empty() ? 1 : 0, nd.name.c_str());
        return 0;
    }
    if (o.aid == "dump-newick") {
        // developer aid (no GPU): the three Newick writers on a log from a text file, tips named t0, t1, ...; the text goes to stdout.
        // First line `nj N last`, then N - 2 lines `x y bx by`; or `upgma N`, then N - 1 lines `x y h`; or `kids N top`, then the
        // 2 (N - 2) children and the 2N - 2 lengths.  Numbers through strtod (hexadecimal floats are read exactly).
        std::ifstream lf(o.aidArg);
        if (!lf) { std::cerr << "ERROR: cant open file: " << o.aidArg << "\n"; return 1; }
        std::string kind, tok;
        long long N = 0;
        if (!(lf >> kind >> N) || N < 2 || N > 100000) die("ERROR: --dump-newick: first line `nj N last`, `upgma N` or `kids N top`");
        auto num = [&]() { if (!(lf >> tok)) die("ERROR: --dump-newick: the file ends early"); return std::strtod(tok.c_str(), nullptr); };
        std::vector<std::string> names;
        for (long long i = 0; i < N; ++i) names.push_back("t" + std::to_string(i));
        const size_t merges = (size_t)(kind == "upgma" ? N - 1 : N - 2);
        std::vector<int32_t> mx(merges), my(merges);
        std::vector<double> a(merges), b(merges);
        if (kind == "nj") {
            const double last = num();
            for (size_t it = 0; it < merges; ++it) { mx[it] = (int32_t)num(); my[it] = (int32_t)num(); a[it] = num(); b[it] = num(); }
            writeNewickFromMerges(std::cout, names, mx, my, a, b, last);
        } else if (kind == "upgma") {
            for (size_t it = 0; it < merges; ++it) { mx[it] = (int32_t)num(); my[it] = (int32_t)num(); a[it] = num(); }
            writeNewickFromUpgma(std::cout, names, mx, my, a);
        } else if (kind == "kids") {
            const int32_t top = (int32_t)num();
            std::vector<int32_t> kids(2 * merges);
            std::vector<double> len((size_t)(2 * N - 2));
            for (int32_t& k : kids) k = (int32_t)num();
            for (double& v : len) v = num();
            writeNewickFromKids(std::cout, names, kids, top, len);
        } else {
            die("ERROR: --dump-newick: first line `nj N last`, `upgma N` or `kids N top`");
        }
        return 0;
    }
    if (o.aid == "dump-lengths") {
        // developer aid (no GPU): every branch-length token of --input-tree, parsed as a double and written back
        // through the number formatter of this build's Newick writers, one per line
        std::ifstream tf(o.treeFile);
        if (!tf) { std::cerr << "ERROR: Unable to open input tree file: " << o.treeFile << "\n"; return 1; }
        std::string nwk;
        std::getline(tf, nwk);
        for (size_t i = 0; i < nwk.size(); ++i) {
            if (nwk[i] != ':') continue;
            char* e = nullptr;
            const double v = std::strtod(nwk.c_str() + i + 1, &e);
            putLength(std::cout, v);
            std::cout << "\n";
        }
        return 0;
    }
    if (o.aid == "dump-packed") {
        // developer aid (no GPU): --dump-packed m|r compares the fast input path (records indexed in the mapped text and
        // packed straight into the flat arrays) with the general one (readSequences + per-sequence encoders)
        const bool aligned = o.aidArg == "m";
        const long long sd = o.seed;
        PackedSequences fast;
        readSequencesPacked(o.inputFile, aligned, sd, fast);
        if (!fast.ok) { std::printf("SERIAL-ONLY\n"); return 0; }
        std::vector<std::string> seqs, names_;
        readSequences(o.inputFile, seqs, names_);
        if (seqs.empty()) { std::printf("0 records\n%s\n", fast.numSequences == 0 ? "IDENTICAL" : "DIFFERENT"); return fast.numSequences == 0 ? 0 : 2; }
        const std::vector<int> ids = shuffledIds(seqs.size(), sd);
        std::vector<std::string> names(seqs.size());
        for (size_t i = 0; i < seqs.size(); ++i) names[(size_t)ids[i]] = names_[i];
        bool same = fast.numSequences == seqs.size() && fast.names == names;
        if (aligned) {
            std::vector<uint64_t> flat; int seqLen = 0;
            packAligned(seqs, ids, flat, seqLen);
            same = same && seqLen == fast.seqLen && flat.size() == fast.flat.size() && std::equal(flat.begin(), flat.end(), fast.flat.begin());
            std::printf("%zu %d %zu\n", seqs.size(), seqLen, flat.size());
        } else {
            std::vector<uint64_t> flat, off, lens;
            packUnaligned(seqs, ids, flat, off, lens);
            same = same && flat.size() == fast.flat.size() && std::equal(flat.begin(), flat.end(), fast.flat.begin()) && off == fast.off && lens == fast.lens;
            std::printf("%zu %zu\n", seqs.size(), flat.size());
        }
        std::printf(same ? "IDENTICAL\n" : "DIFFERENT\n");
        return same ? 0 : 2;
    }
    if (o.aid == "dump-jplace") {
        // developer aid (no GPU): the jplace writer on rows from a text file.  --dump-jplace FILE with --input-tree; FILE holds per
        // query a line `NAME K` and K lines `EDGE COUNT DISTAL PENDANT` (strtod: nan and inf are read as such); --bootstrap N sets
        // the replicates, --site-coverage X the threshold named in the metadata.  The file goes to stdout.
        std::ifstream tf(o.treeFile);
        if (!tf) { std::cerr << "ERROR: Unable to open input tree file: " << o.treeFile << "\n"; return 1; }
        std::string nwk;
        std::getline(tf, nwk);
        std::ifstream rf(o.aidArg);
        if (!rf) { std::cerr << "ERROR: cant open file: " << o.aidArg << "\n"; return 1; }
        std::vector<std::string> qnames;
        std::vector<std::vector<PlacementRow>> rows;
        std::string nm;
        size_t k = 0;
        while (rf >> nm >> k) {
            qnames.push_back(nm);
            rows.emplace_back();
            for (size_t i = 0; i < k; ++i) {
                std::string e, c, d, pl;
                if (!(rf >> e >> c >> d >> pl)) die("ERROR: --dump-jplace: a row has four fields");
                rows.back().push_back(PlacementRow{ (int32_t)std::stol(e), std::stoll(c), std::strtod(d.c_str(), nullptr), std::strtod(pl.c_str(), nullptr) });
            }
        }
        Tree t(nwk, 0);
        std::vector<std::string> names(t.m_numLeaves, "");
        names.insert(names.end(), qnames.begin(), qnames.end());
        Param params;
        params.in = "m";
        params.distanceType = o.params.distanceType;
        BootstrapOptions bo;
        bo.replicates = o.boot.replicates;
        // (--site-coverage X: the two metadata fields of a filtered run, with no site counted: sites_kept 0)
        if (o.sitePermille) params.siteCoverage = o.siteText;
        writeJplace(std::cout, t, names, rows, params, bo);
        return 0;
    }
    if (o.aid == "dump-fasta") {
        // developer aid (no GPU): read --input-file and print name, length and FNV-1a of every record
        std::vector<std::string> seqs, names;
        readSequences(o.inputFile, seqs, names);
        std::printf("%zu\n", seqs.size());
        for (size_t i = 0; i < seqs.size(); ++i) {
            uint64_t h = 1469598103934665603ull;
            for (unsigned char ch : seqs[i]) { h ^= ch; h *= 1099511628211ull; }
            std::printf("%s %zu %016llx\n", names[i].c_str(), seqs[i].size(), (unsigned long long)h);
        }
        return 0;
    }
    return 0;
}

}  // namespace dipper
