// dipper -- what the command line means: the flags and the help of the reference's main() (src/tree_generation.cu:33-99,159-230)
// and this build's own options, parsed and checked in one place.  The order of the checks is the order of the messages a caller
// sees when two rules are broken (tests/golden/cli_usage_matrix.tsv).
#include "options.hpp"

#include <cctype>
#include <iostream>
#include <map>

namespace dipper {

const char* const kHelp =
    "DIPPER Command Line Arguments:\n\n"
    "Required Options:\n"
    "  -i [ --input-format ] arg   Input format:\n"
    "                                d - distance matrix in PHYLIP format\n"
    "                                r - unaligned sequences in FASTA format\n"
    "                                m - aligned sequences in FASTA format\n"
    "  -I [ --input-file ] arg     Input file path:\n"
    "                                PHYLIP format for distance matrix\n"
    "                                FASTA format for aligned or unaligned sequences\n"
    "  -O [ --output-file ] arg    Output file path\n\n"
    "Optional Options:\n"
    "  -o [ --output-format ] arg  Output format:\n"
    "                                t - phylogenetic tree in Newick format (default)\n"
    "                                d - distance matrix in PHYLIP format (coming soon)\n"
    "                                j - placements in jplace format: every query placed on the\n"
    "                                    backbone by itself, the backbone unchanged (needs --add -t,\n"
    "                                    -i m or -i r; with --bootstrap: placement support per edge)\n"
    "                                p - the pairs of sequences within a distance threshold (needs --within;\n"
    "                                    -i m, r or d), as a table; no tree and no matrix is built\n"
    "                                n - the nearest neighbours of every sequence (needs --nearest; -i m, r or\n"
    "                                    d), as a table; no tree and no matrix is built\n"
    "                                s - the minimum spanning tree of the distances (-i m, r or d), as a table of\n"
    "                                    its edges; no matrix is built\n"
    "  -m [ --algorithm ] arg      Algorithm selection:\n"
    "                                0 - default mode\n"
    "                                1 - force placement\n"
    "                                2 - force conventional NJ\n"
    "                                3 - force divide-and-conquer\n"
    "  -p [ --placement-mode ] arg Placement mode:\n"
    "                                0 - exact mode\n"
    "                                1 - k-closest mode (default)\n"
    "  -k [ --kmer-size ] arg      K-mer size:\n"
    "                                Valid range: 2-15 (default: 15)\n"
    "  -s [ --sketch-size ] arg    Sketch size (default: 1000)\n"
    "  -d [ --distance-type ] arg  Distance type to calculate:\n"
    "                                1 - uncorrected\n"
    "                                2 - JC (default)\n"
    "                                3 - Tajima-Nei\n"
    "                                4 - K2P\n"
    "                                5 - Tamura\n"
    "                                6 - Jinnei\n"
    "                                7 - Poisson correction (--protein only)\n"
    "                                8 - Kimura 1983 (--protein only)\n"
    "                                9 - TN93 (Tamura-Nei 1993; nucleotides only, as are 10 and 11)\n"
    "                                10 - LogDet\n"
    "                                11 - paralinear\n"
    "  -a [ --add ]                Add query to backbone using k-closest placement\n"
    "  -t [ --input-tree ] arg     Input backbone tree (Newick format), required with --add option\n"
    "  -h [ --help ]               Print this help message\n\n"
    "MI355X build options:\n"
    "  --seed arg                  Seed of the input-order shuffle (reference: time(NULL));\n"
    "                              default 1, negative keeps the input order\n"
    "  --device arg                GPU index (default 0; the reference hard-codes 1)\n"
    "  --gpus arg                  Number of GPUs: one rank process per GPU, started by this command\n"
    "                              once the input is read (devices --device, --device+1, ...)\n"
    "  --devices arg               Comma-separated GPU index of every rank (the same index twice:\n"
    "                              ranks share that GPU -- rehearsal of the multi-GPU paths)\n"
    "  --transport arg             auto (default) | rccl | ipc: how the ranks exchange data\n"
    "  --rank arg --world arg --rendezvous arg\n"
    "                              this process is rank `rank` of `world` ranks started from outside;\n"
    "                              they meet in the POSIX shared memory object `rendezvous`\n"
    "  --protein                   The alignment holds amino acids (-i m only): the 20 letters\n"
    "                              ARNDCQEGHILKMFPSTWYV in either case, anything else is a gap; distances\n"
    "                              over the sites where both sequences hold a residue.  -d 1 (p-distance,\n"
    "                              default), 2 (JC with 20 states), 7 or 8; conventional NJ, placement,\n"
    "                              --add and -o d / -o j; not with --bootstrap or divide-and-conquer\n"
    "  --site-coverage arg         Keep only the alignment columns in which at least arg of the sequences hold\n"
    "                              a symbol (A, C, G, T/U; with --protein one of the 20 residues): a decimal\n"
    "                              0 < arg <= 1 with at most three places; a column exactly at the threshold\n"
    "                              is kept (partial deletion; without the option every pair of sequences\n"
    "                              uses the sites it has: pairwise deletion).  The columns are counted and\n"
    "                              removed on the GPU after the upload; everything else runs on the filtered\n"
    "                              alignment.  -i m only; every -d, -m and -o, --protein, --bionj, --nni,\n"
    "                              --spr, --upgma, --wpgma, --bootstrap (replicates resample the filtered\n"
    "                              alignment), --gpus / --devices.  With --add the coverage is taken over\n"
    "                              all sequences of the input file, backbone and queries together.  No\n"
    "                              column kept: an error, no output file\n"
    "  --complete-deletion         As --site-coverage 1: only the columns without any gap or ambiguity code\n"
    "                              (complete deletion).  Not together with --site-coverage\n"
    "  --bionj                     Build the tree with BIONJ (Gascuel 1997) instead of NJ: the same pair\n"
    "                              selection and branch lengths; the distances of a new node are a\n"
    "                              variance-weighted mean of its children's.  Wherever conventional NJ\n"
    "                              builds the tree (-m 2, or -m 0 below 30000; -i d, m or r; --protein;\n"
    "                              every -d); with --bootstrap the main tree and every replicate tree are\n"
    "                              BIONJ trees.  Not with -m 1, -m 3, --add, -o d or -o j\n"
    "  --nni arg                   Refine the NJ / BIONJ tree by nearest-neighbour interchanges under balanced\n"
    "                              minimum evolution (Desper & Gascuel 2002): at most arg >= 0 rounds, each\n"
    "                              applying every improving interchange that shares no node with a better\n"
    "                              one; the tree is written with its balanced branch lengths (arg 0: those of\n"
    "                              the NJ topology).  Wherever conventional NJ builds the tree (-m 2, or -m 0\n"
    "                              below 30000; -i d, m or r; --protein; --bionj; every -d); one GPU.  Not\n"
    "                              with -m 1, -m 3, --add, -o d, -o j, --bootstrap or several ranks\n"
    "  --spr arg                   As --nni, with subtree pruning and regrafting moves: a subtree may be carried\n"
    "                              past any number of edges in one move (an interchange is the move past one),\n"
    "                              which leaves optima that hold --nni.  At most arg >= 0 rounds, each applying\n"
    "                              every improving move that shares no node with a better one.  Valid where\n"
    "                              --nni is; not together with --nni\n"
    "  --upgma                     Build a rooted, ultrametric tree by UPGMA (average linkage: the distance of two\n"
    "                              clusters is the mean over their pairs of tips) instead of NJ; the tree is\n"
    "                              written rooted, `(A:l,B:l);`, every tip at the same distance from the root.\n"
    "                              Wherever conventional NJ builds the tree (-m 2, or -m 0 below 30000; -i d,\n"
    "                              m or r; --protein; every -d); one GPU; with --bootstrap the main tree and\n"
    "                              every replicate tree are UPGMA trees.  Not with --bionj, --nni, --spr,\n"
    "                              -m 1, -m 3, --add, -o d, -o j or several ranks\n"
    "  --wpgma                     As --upgma with WPGMA: a merged cluster's distances are the plain mean of\n"
    "                              its two parts' (McQuitty's weighted linkage).  Not together with --upgma\n"
    "  --fit                       After the tree is written, report how well it explains the distances: over all\n"
    "                              pairs of taxa the residual of the distance against the tree's path length --\n"
    "                              one line `Fit:` on stderr with the pairs counted (a pair with a non-finite\n"
    "                              distance or path length is skipped), the sum of squares, the rms residual, the\n"
    "                              relative rms (PHYLIP's average percent standard deviation / 100), the explained\n"
    "                              variance (FastME), the cophenetic correlation and the worst pair; a second line\n"
    "                              names the five taxa with the largest rms residual.  Computed on the GPU from a\n"
    "                              fresh distance matrix; the tree file is unchanged.  Valid where --nni is (-m 2,\n"
    "                              or -m 0 below 30000; -i d, m or r; --protein; every -d; --site-coverage; one\n"
    "                              GPU), with --bionj, --nni, --spr, --upgma and --wpgma.  Not with -m 1, -m 3,\n"
    "                              --add, -o d, -o j, --bootstrap or several ranks\n"
    "  --fit-taxa arg              Write the per-taxon residuals to file arg: a header line, then for every taxon\n"
    "                              in input order its counted pairs, residual sum of squares, rms residual and\n"
    "                              that rms over the tree-wide rms (tab-separated, 17 significant digits).\n"
    "                              Needs --fit\n"
    "  --within arg                With -o p: the distance threshold T, a decimal >= 0.  The output file gets the\n"
    "                              line `ID1<TAB>ID2<TAB>Distance`, then one line per pair of sequences whose\n"
    "                              distance d -- the number -o d prints for the pair -- is <= T (a distance\n"
    "                              that is not a number or infinite never is), ordered by the later sequence\n"
    "                              of the pair in input order, then by the earlier one; input order is kept\n"
    "                              (--seed, -m and -p are not consulted).  The distances are computed on the\n"
    "                              GPU a block of rows at a time and filtered there: the matrix is never held,\n"
    "                              so inputs far beyond the reach of -o d work.  One line `Pairs:` on stderr.\n"
    "                              -i m with every -d, --protein, --site-coverage / --complete-deletion; -i r\n"
    "                              with -k / -s; -i d; one GPU.  Not with --add, -t or a tree option\n"
    "  --clusters arg              With -o p: write the single-linkage clusters at T -- the connected components\n"
    "                              of the pairs -- to file arg: a `#` line with the totals, then every sequence\n"
    "                              in input order with the number of its cluster (clusters numbered from 1 by\n"
    "                              their first sequence).  Computed on the GPU\n"
    "  --nearest arg               With -o n: the number K of neighbours, a whole number from 1 to 256.  The output\n"
    "                              file gets the line `ID<TAB>Rank<TAB>Neighbour<TAB>Distance`, then for every\n"
    "                              sequence in input order its K nearest sequences, nearest first (rank 1, 2,\n"
    "                              ...; equal distances in input order), with the distance -o d prints for the\n"
    "                              pair.  A distance that is not a number or infinite makes no neighbour: a\n"
    "                              sequence may have fewer than K lines, or none.  Input order is kept (--seed,\n"
    "                              -m and -p are not consulted).  The distances are computed on the GPU a block\n"
    "                              of rows at a time and the K best of every row are selected there: the matrix\n"
    "                              is never held.  One line `Nearest:` on stderr.  Valid where -o p is: -i m with\n"
    "                              every -d, --protein, --site-coverage / --complete-deletion; -i r with -k /\n"
    "                              -s; -i d; one GPU.  Not with --add, -t, a tree option, --within or --clusters\n"
    "  --dendrogram arg            With -o s: write the single-linkage dendrogram to file arg, a rooted ultrametric\n"
    "                              tree in Newick format (an edge of the spanning tree joins its two sides at\n"
    "                              half its distance).  When the distances leave several components there is\n"
    "                              no such tree: the edge file is written, the reason goes to stderr and the\n"
    "                              exit status is 1.  -o s itself: the output file gets the line\n"
    "                              `ID1<TAB>ID2<TAB>Distance`, then one line per edge of the minimum spanning\n"
    "                              tree (of every component, when a distance that is not a number or infinite\n"
    "                              separates some), shortest first, equal distances by the later sequence of\n"
    "                              the pair in input order and then the earlier one, with the distance -o d\n"
    "                              prints for the pair.  Cutting the list at a distance T gives the clusters\n"
    "                              of -o p --within T.  Input order is kept (--seed, -m and -p are not\n"
    "                              consulted).  The distances are computed on the GPU a block of rows at a\n"
    "                              time, once per round of Boruvka's algorithm: the matrix is never held.  One\n"
    "                              line `MST:` on stderr.  Valid where -o n is: -i m with every -d, --protein,\n"
    "                              --site-coverage / --complete-deletion; -i r with -k / -s; -i d; one GPU.\n"
    "                              Not with --add, -t, a tree option, --within, --clusters or --nearest\n"
    "  --bootstrap arg             Felsenstein bootstrap: arg >= 1 replicate alignments (columns drawn\n"
    "                              with replacement); the NJ tree's internal nodes are labelled with\n"
    "                              the percentage of replicate trees that hold their split.\n"
    "                              -i m -o t with conventional NJ only (-m 2, or -m 0 below 30000)\n"
    "                              With --add -o j -i m: the queries are placed again under every\n"
    "                              replicate alignment; like_weight_ratio = share of replicates per edge\n"
    "  --bootstrap-seed arg        Seed of the replicates' column draws (unsigned 64-bit, default 1)\n"
    "  --bootstrap-metric arg      fbp (default): Felsenstein support, the share of replicates that hold\n"
    "                              a split exactly; tbe: transfer bootstrap expectation, one minus the\n"
    "                              mean share of a split's taxa that must move to reach a replicate\n"
    "  --bootstrap-taxa arg        Write the per-taxon transfer index (rogue taxa) to file arg: for every\n"
    "                              taxon, in input order, the number and the share of the (branch,\n"
    "                              replicate) pairs in which it must move to reach the closest replicate\n"
    "                              branch.  Needs --bootstrap; either metric; the tree file is unchanged\n"
    "  --bootstrap-taxa-cutoff arg Count a (branch, replicate) pair when its transfer distance is at most\n"
    "                              arg x (p - 1): a decimal 0 <= arg < 1 with at most three places\n"
    "                              (default 0.3).  Needs --bootstrap-taxa\n";

struct Opt { const char* lng; char sht; bool has_arg; };
static const Opt kOpts[] = {
    { "input-format", 'i', true }, { "input-file", 'I', true }, { "output-file", 'O', true },
    { "output-format", 'o', true }, { "algorithm", 'm', true }, { "placement-mode", 'p', true },
    { "kmer-size", 'k', true }, { "sketch-size", 's', true }, { "distance-type", 'd', true },
    { "add", 'a', false }, { "input-tree", 't', true }, { "help", 'h', false },
    { "seed", 0, true }, { "device", 0, true }, { "gpus", 0, true }, { "devices", 0, true }, { "transport", 0, true },
    { "rank", 0, true }, { "world", 0, true }, { "rendezvous", 0, true }, { "dump-tree", 0, true }, { "dump-fasta", 0, false }, { "dump-lengths", 0, false }, { "dump-packed", 0, true }, { "dump-jplace", 0, true },
    { "bootstrap", 0, true }, { "bootstrap-seed", 0, true }, { "bootstrap-metric", 0, true },
    { "bootstrap-taxa", 0, true }, { "bootstrap-taxa-cutoff", 0, true }, { "protein", 0, false },
    { "bionj", 0, false }, { "nni", 0, true }, { "spr", 0, true }, { "upgma", 0, false }, { "wpgma", 0, false },
    { "site-coverage", 0, true }, { "complete-deletion", 0, false }, { "fit", 0, false }, { "fit-taxa", 0, true }, { "dump-newick", 0, true },
    { "within", 0, true }, { "clusters", 0, true }, { "nearest", 0, true }, { "dendrogram", 0, true },
};

static void usageError(const std::string& what)
{
    std::cerr << "\033[31m" << what << "\033[0m" << std::endl;
    std::cerr << kHelp << std::endl;
    std::exit(1);
}

static std::map<std::string, std::string> parseArguments(int argc, char** argv)
{
    std::map<std::string, std::string> vm;
    for (int a = 1; a < argc; ++a) {
        std::string tok = argv[a];
        const Opt* opt = nullptr;
        std::string val;
        bool have_val = false;
        if (tok.rfind("--", 0) == 0) {
            std::string nm = tok.substr(2);
            const size_t eq = nm.find('=');
            if (eq != std::string::npos) { val = nm.substr(eq + 1); nm = nm.substr(0, eq); have_val = true; }
            for (const Opt& o : kOpts) if (nm == o.lng) opt = &o;
            if (!opt) usageError("unrecognised option '" + tok + "'");
        } else if (tok.size() >= 2 && tok[0] == '-') {
            for (const Opt& o : kOpts) if (o.sht && tok[1] == o.sht) opt = &o;
            if (!opt) usageError("unrecognised option '" + tok + "'");
            if (tok.size() > 2) { val = tok.substr(2); have_val = true; }
        } else {
            usageError("too many positional options have been specified on the command line");
        }
        if (opt->has_arg) {
            if (!have_val) {
                if (a + 1 >= argc) usageError(std::string("the required argument for option '--") + opt->lng + "' is missing");
                val = argv[++a];
            }
            vm[opt->lng] = val;
        } else {
            vm[opt->lng] = "1";
        }
    }
    return vm;
}

static uint64_t stoiOr(const std::map<std::string, std::string>& vm, const char* key, uint64_t dflt)
{
    // the reference parses every numeric flag with stoi inside try{}catch{} (src/tree_generation.cu:191-208)
    auto it = vm.find(key);
    if (it == vm.end()) return dflt;
    try { return (uint64_t)std::stoi(it->second); } catch (...) { return dflt; }
}

static std::string strOr(const std::map<std::string, std::string>& vm, const char* key, const std::string& dflt)
{
    auto it = vm.find(key);
    return it == vm.end() ? dflt : it->second;
}

using Args = std::map<std::string, std::string>;
static const char* const kNeedsNJ = " needs conventional NJ";

// --bootstrap and its companions: what the arguments alone decide
static void parseBootstrap(const Args& vm, Options& o)
{
    BootstrapOptions& boot = o.boot;
    if (vm.count("bootstrap-seed") && !vm.count("bootstrap")) usageError("--bootstrap-seed needs --bootstrap");
    if (vm.count("bootstrap-metric") && !vm.count("bootstrap")) usageError("--bootstrap-metric needs --bootstrap");
    if (vm.count("bootstrap-taxa") && !vm.count("bootstrap")) usageError("--bootstrap-taxa needs --bootstrap");
    if (vm.count("bootstrap-taxa-cutoff") && !vm.count("bootstrap-taxa")) usageError("--bootstrap-taxa-cutoff needs --bootstrap-taxa");
    if (!vm.count("bootstrap")) return;
    auto whole = [](const std::string& v, bool sign_ok) {
        if (v.empty() || v.size() > 20) return false;
        for (size_t i = 0; i < v.size(); ++i)
            if (!std::isdigit((unsigned char)v[i]) && !(sign_ok && i == 0 && (v[i] == '-' || v[i] == '+') && v.size() > 1)) return false;
        return true;
    };
    const std::string nv = vm.at("bootstrap");
    long long nr = 0;
    try { nr = whole(nv, true) ? std::stoll(nv) : 0; } catch (...) { nr = 0; }
    if (nr <= 0 || nr > (1ll << 30)) usageError("--bootstrap: the number of replicates must be a whole number >= 1");
    boot.replicates = nr;
    if (vm.count("bootstrap-seed")) {
        const std::string sv = vm.at("bootstrap-seed");
        try {
            if (!whole(sv, false)) throw 0;
            boot.seed = (uint64_t)std::stoull(sv);
        } catch (...) { usageError("--bootstrap-seed: an unsigned 64-bit integer"); }
    }
    if (vm.count("bootstrap-metric")) {
        const std::string mv = vm.at("bootstrap-metric");
        if (mv != "fbp" && mv != "tbe") usageError("--bootstrap-metric: fbp or tbe");
        boot.tbe = mv == "tbe";
    }
    if (vm.count("bootstrap-taxa")) {
        o.bootTaxaFile = vm.at("bootstrap-taxa");
        if (o.bootTaxaFile.empty()) usageError("--bootstrap-taxa: a file name");
        if (o.bootTaxaFile == o.outputFile) usageError("--bootstrap-taxa: the file must differ from the output file (-O)");
    }
    if (vm.count("bootstrap-taxa-cutoff")) {
        // per mille from the text: 0, 0.3, .25, 0.125 -- digits, at most one point, at most three places, an integer part of 0
        const std::string cv = vm.at("bootstrap-taxa-cutoff");
        const size_t dot = cv.find('.');
        const std::string ip = cv.substr(0, dot), fp = dot == std::string::npos ? "" : cv.substr(dot + 1);
        bool ok = !cv.empty() && (!ip.empty() || !fp.empty()) && fp.size() <= 3 && ip.size() <= 20;
        for (char ch : ip) ok = ok && ch == '0';
        for (char ch : fp) ok = ok && std::isdigit((unsigned char)ch);
        if (!ok) usageError("--bootstrap-taxa-cutoff: a decimal 0 <= x < 1 with at most three places (0.3)");
        int pm = 0;
        for (size_t i = 0; i < 3; ++i) pm = 10 * pm + (i < fp.size() ? fp[i] - '0' : 0);
        boot.taxaCutoff = pm;
    }
    if (o.params.in != "m") usageError("--bootstrap needs aligned sequences (-i m)");
    if (o.add && !o.jplace) usageError("--bootstrap is not supported with --add");
    if (o.params.out != "t" && !o.jplace) usageError("--bootstrap needs tree output (-o t)");
    if (o.jplace) return;      // (placement support: no tree is built)
    if (o.algo == "1" || o.algo == "3") usageError(std::string("--bootstrap") + kNeedsNJ + " (-m 2, or the default mode below 30000 sequences)");
    o.njOnly = std::string("--bootstrap") + kNeedsNJ;      // (named before the tree builders' own)
}

// several GPUs: one rank process per GPU, started once the input is read and before the first GPU call (startRanks)
static void parseRanks(const Args& vm, Options& o)
{
    RankOptions& ranks = o.ranks;
    ranks.gpus = (int)stoiOr(vm, "gpus", 1);
    if (ranks.gpus < 1) usageError("--gpus must be at least 1");
    if (vm.count("devices")) {
        std::stringstream ss(vm.at("devices"));
        std::string tok;
        while (std::getline(ss, tok, ',')) {
            try { ranks.devices.push_back(std::stoi(tok)); } catch (...) { usageError("--devices: a comma-separated list of GPU indices"); }
        }
        if (!vm.count("gpus") && !vm.count("world")) ranks.gpus = (int)ranks.devices.size();
    }
    const std::string tr = strOr(vm, "transport", "auto");
    if (tr == "auto") ranks.transport = 0; else if (tr == "rccl") ranks.transport = 1; else if (tr == "ipc") ranks.transport = 2;
    else usageError("--transport: auto, rccl or ipc");
    if (vm.count("world")) {
        ranks.ext_world = (int)stoiOr(vm, "world", 1);
        ranks.ext_rank = vm.count("rank") ? (int)stoiOr(vm, "rank", 0) : -1;
        ranks.rendezvous = strOr(vm, "rendezvous", "");
        ranks.gpus = 1;
        if (ranks.ext_world > 1 && (ranks.ext_rank < 0 || ranks.ext_rank >= ranks.ext_world || ranks.rendezvous.empty()))
            usageError("--world needs --rank (0 <= rank < world) and --rendezvous");
    }
    o.multi = ranks.multi();
}

Options parseOptions(int argc, char** argv)
{
    const Args vm = parseArguments(argc, argv);
    auto has = [&](const char* key) { return vm.count(key) != 0; };
    Options o;
    o.help = has("help");
    if (o.help) return o;
    Param& params = o.params;
    o.inputFile = strOr(vm, "input-file", "");
    o.outputFile = strOr(vm, "output-file", "");
    o.treeFile = strOr(vm, "input-tree", "");
    params.distanceType = stoiOr(vm, "distance-type", 1);  // code default is 1 although the help says JC
    try { if (has("seed")) o.seed = std::stoll(vm.at("seed")); } catch (...) {}
    for (const char* aid : { "dump-tree", "dump-newick", "dump-lengths", "dump-packed", "dump-jplace", "dump-fasta" }) {
        if (!has(aid)) continue;
        // a developer aid (the first of the six in this order): what its body reads beyond the above, unchecked
        o.aid = aid;
        o.aidArg = vm.at(aid);
        o.boot.replicates = (int64_t)stoiOr(vm, "bootstrap", 0);
        o.sitePermille = has("site-coverage") ? parseSiteCoverage(vm.at("site-coverage")) : 0;
        if (o.sitePermille) o.siteText = siteCoverageText(o.sitePermille);
        return o;
    }
    for (const char* req : { "input-format", "input-file", "output-file" })
        if (!has(req)) usageError(std::string("the option '--") + req + "' is required but missing");
    params.in = vm.at("input-format");
    params.out = strOr(vm, "output-format", "t");
    o.algo = strOr(vm, "algorithm", "0");
    o.add = has("add");

    // Everything below is what the arguments alone decide, before any input is read or a GPU touched.
    // The rules the tree-builder options share, written once: conventional NJ only, no --add, -o t only, optionally no --bootstrap
    // (with the reason), and -- checked last of all, once the rank options are parsed -- one GPU
    std::vector<std::string> oneGpu;
    auto treeBuilder = [&](const std::string& label, const char* wording, const char* noBootstrap, bool one_gpu) {
        if (o.algo == "1" || o.algo == "3") usageError(label + wording + " (-m 2, or the default mode below 30000 sequences)");
        if (o.add) usageError(label + " is not supported with --add");
        if (params.out == "d" || params.out == "j" || params.out == "p" || params.out == "n" || params.out == "s") usageError(label + " needs tree output (-o t)");
        if (noBootstrap && has("bootstrap")) usageError(label + " is not supported with --bootstrap (" + noBootstrap + ")");
        if (o.njOnly.empty()) o.njOnly = label + wording;
        if (one_gpu) oneGpu.push_back(label);
    };
    o.bionj = has("bionj");
    if (o.bionj) treeBuilder("--bionj", kNeedsNJ, nullptr, false);
    o.spr = has("spr");
    const std::string refine = o.spr ? "--spr" : "--nni";
    if (o.spr && has("nni")) usageError("--spr is not supported with --nni (an SPR search contains the NNI moves)");
    if (has("nni") || o.spr) {
        const std::string nv = vm.at(o.spr ? "spr" : "nni");
        bool digits = !nv.empty() && nv.size() <= 9;
        for (char ch : nv) digits = digits && std::isdigit((unsigned char)ch);
        if (!digits) usageError(refine + ": the number of rounds must be a whole number >= 0");
        o.nni = std::stoi(nv);
        treeBuilder(refine, kNeedsNJ, "replicate trees are not refined", true);
    }
    o.upgma = has("upgma") ? 0 : has("wpgma") ? 1 : -1;
    if (o.upgma >= 0) {
        const std::string cluster = o.upgma == 1 ? "--wpgma" : "--upgma";
        if (has("upgma") && has("wpgma")) usageError("--upgma is not supported with --wpgma (one linkage a tree)");
        if (o.bionj) usageError(cluster + " is not supported with --bionj (it builds the tree in place of NJ / BIONJ)");
        if (o.nni >= 0) usageError(cluster + " is not supported with " + refine + " (a rooted ultrametric tree is not refined)");
        treeBuilder(cluster, " builds the tree where conventional NJ does", nullptr, true);
    }
    o.fit = has("fit");
    if (has("fit-taxa") && !o.fit) usageError("--fit-taxa needs --fit");
    if (o.fit) {
        treeBuilder("--fit", kNeedsNJ, "one tree, one matrix", true);
        if (has("fit-taxa")) {
            o.fitTaxaFile = vm.at("fit-taxa");
            if (o.fitTaxaFile.empty()) usageError("--fit-taxa: a file name");
            if (o.fitTaxaFile == o.outputFile) usageError("--fit-taxa: the file must differ from the output file (-O)");
        }
    }
    if (o.add && !has("input-tree"))
        usageError("Backbone tree (--input-tree/-t) is required with --add option");
    o.protein = params.protein = has("protein");
    if (o.protein) {
        if (params.in != "m") usageError("--protein needs aligned sequences (-i m)");
        const uint64_t dt = params.distanceType;
        if (dt >= DPR_DIST_TAJIMANEI && dt <= DPR_DIST_JINNEI) usageError("-d 3 to 6 are nucleotide models: --protein takes -d 1, 2, 7 or 8");
        if (dt != DPR_DIST_UNCORRECTED && dt != DPR_DIST_JC && dt != DPR_DIST_POISSON && dt != DPR_DIST_KIMURA) usageError("--protein takes -d 1, 2, 7 or 8");
        if (has("bootstrap")) usageError("--bootstrap is not available with --protein (nucleotide alignments only)");
        if (o.algo == "3") usageError("divide-and-conquer (-m 3) is not available with --protein; use -m 1 or -m 2");
    }
    if (has("site-coverage") || has("complete-deletion")) {
        if (has("site-coverage") && has("complete-deletion"))
            usageError("--complete-deletion is --site-coverage 1: give one of the two");
        if (params.in != "m") usageError("--site-coverage / --complete-deletion need aligned sequences (-i m)");
        o.sitePermille = has("complete-deletion") ? 1000 : parseSiteCoverage(vm.at("site-coverage"));
        if (o.sitePermille < 1) usageError("--site-coverage: a decimal 0 < x <= 1 with at most three places (0.5)");
        o.siteText = siteCoverageText(o.sitePermille);
    }
    // -o j: placements on a fixed backbone
    o.jplace = params.out == "j";
    if (o.jplace) {
        if (!o.add) usageError("-o j needs --add and a backbone tree (-t): the queries are placed on that tree");
        if (params.in != "m" && params.in != "r") usageError("-o j needs aligned or unaligned sequences (-i m or -i r)");
        if (has("bootstrap") && params.in != "m") usageError("--bootstrap with -o j needs aligned sequences (-i m)");
        if (has("bootstrap-metric")) usageError("--bootstrap-metric does not apply to -o j (placement support is the share of replicates per edge)");
        if (has("bootstrap-taxa") || has("bootstrap-taxa-cutoff")) usageError("--bootstrap-taxa does not apply to -o j");
    }
    // -o p: the pairs within a threshold
    o.pairs = params.out == "p";
    if (has("within") && !o.pairs) usageError("--within needs the pair output (-o p)");
    if (has("clusters") && !o.pairs) usageError("--clusters needs the pair output (-o p)");
    if (o.pairs) {
        if (!has("within")) usageError("-o p needs a distance threshold (--within T)");
        // a finite decimal >= 0 that strtod consumes whole (no leading blank, no hexadecimal, no `inf` / `nan`)
        o.withinText = vm.at("within");
        const std::string& wv = o.withinText;
        bool plain = !wv.empty() && wv.size() <= 64;
        for (char ch : wv) plain = plain && (std::isdigit((unsigned char)ch) || ch == '.' || ch == 'e' || ch == 'E' || ch == '+' || ch == '-');
        char* endp = nullptr;
        o.within = plain ? std::strtod(wv.c_str(), &endp) : -1.0;
        if (!plain || endp != wv.c_str() + wv.size() || !(o.within >= 0.0) || !std::isfinite(o.within))
            usageError("--within: the threshold must be a finite decimal >= 0 (0.015)");
        if (o.add || has("input-tree")) usageError("-o p is not supported with --add or -t (it compares the sequences of one input with each other)");
        if (has("bootstrap")) usageError("--bootstrap needs tree output (-o t)");
        if (has("clusters")) {
            o.clustersFile = vm.at("clusters");
            if (o.clustersFile.empty()) usageError("--clusters: a file name");
            if (o.clustersFile == o.outputFile) usageError("--clusters: the file must differ from the output file (-O)");
        }
        oneGpu.push_back("-o p");
    }
    // -o n: the nearest neighbours of every sequence
    o.nearest = params.out == "n";
    if (has("nearest") && !o.nearest) usageError("--nearest needs the neighbour output (-o n)");
    if (o.nearest) {
        if (!has("nearest")) usageError("-o n needs the number of neighbours (--nearest K)");
        const std::string& kv = vm.at("nearest");
        bool digits = !kv.empty() && kv.size() <= 9;
        for (char ch : kv) digits = digits && std::isdigit((unsigned char)ch);
        o.nearestK = digits ? std::stoi(kv) : 0;
        if (o.nearestK < 1 || o.nearestK > DPR_NEAREST_MAX_K) usageError("--nearest: the number of neighbours must be a whole number from 1 to 256");
        if (o.add || has("input-tree")) usageError("-o n is not supported with --add or -t (it compares the sequences of one input with each other)");
        if (has("bootstrap")) usageError("--bootstrap needs tree output (-o t)");
        oneGpu.push_back("-o n");
    }
    // -o s: the minimum spanning tree of the distances
    o.mst = params.out == "s";
    if (has("dendrogram") && !o.mst) usageError("--dendrogram needs the spanning-tree output (-o s)");
    if (o.mst) {
        if (o.add || has("input-tree")) usageError("-o s is not supported with --add or -t (it compares the sequences of one input with each other)");
        if (has("bootstrap")) usageError("--bootstrap needs tree output (-o t)");
        if (has("dendrogram")) {
            o.dendrogramFile = vm.at("dendrogram");
            if (o.dendrogramFile.empty()) usageError("--dendrogram: a file name");
            if (o.dendrogramFile == o.outputFile) usageError("--dendrogram: the file must differ from the output file (-O)");
        }
        oneGpu.push_back("-o s");
    }
    parseBootstrap(vm, o);

    params.kmerSize = stoiOr(vm, "kmer-size", 15);
    params.sketchSize = stoiOr(vm, "sketch-size", 1000);
    const std::string placemode = strOr(vm, "placement-mode", "1");  // the reference reads --algorithm here
    // exact placement mode: `-p 0`, or -- the reference's effective behaviour, which reads the placement mode
    // from --algorithm (src/tree_generation.cu:222-224) -- an explicit `-m 0` that lands in placement
    o.exact_mode = placemode == "0" || (has("algorithm") && o.algo == "0");
    o.device = (int)stoiOr(vm, "device", 0);
    parseRanks(vm, o);
    const bool several = o.multi || o.ranks.devices.size() > 1 || has("rank") || has("world");
    for (const std::string& label : oneGpu)
        if (several) usageError(label + " runs on one GPU (not with --gpus above 1, several --devices or --rank / --world)");
    if (!o.multi && o.ranks.devices.size() == 1) o.device = o.ranks.devices[0];      // (`--devices 3` alone: one rank on GPU 3)
    return o;
}

void applyOptions(const Options& o)
{
    bionjOption() = o.bionj;      // every context of this command builds BIONJ trees (DeviceContext, the bootstrap's rank-local one)
    if (o.upgma >= 0) upgmaOption() = o.upgma;
    fitOption().on = o.fit;
    fitOption().taxaFile = o.fitTaxaFile;
    if (o.sitePermille) {
        SiteFilterOption& sf = siteFilterOption();      // every alignment this command uploads is filtered (MSADeviceArrays, the bootstrap's rank-local context)
        sf.permille = o.sitePermille;
        sf.text = o.siteText;
        sf.outputFile = o.outputFile;
    }
}

int pickMode(const Options& o, long long n)
{
    const long long placement_thr = 30000, dc_thr = 1000000;  // src/tree_generation.cu:247-248
    if (o.algo == "1" || (o.algo == "0" && n >= placement_thr && n < dc_thr)) return 1;
    if (o.algo == "3" || (o.algo == "0" && n >= dc_thr)) return 3;
    return 2;
}

int checkedMode(const Options& o, long long n)
{
    const int mode = pickMode(o, n);
    if (mode != 2 && !o.njOnly.empty())
        die("ERROR: " + o.njOnly + ": " + std::to_string(n) + " sequences select " +
            (mode == 1 ? "placement" : "divide-and-conquer") + " in the default mode; use -m 2");
    if (o.protein && mode == 3)
        die("ERROR: divide-and-conquer is not available with --protein: " + std::to_string(n) +
            " sequences select it in the default mode; use -m 1 or -m 2");
    return mode;
}

}  // namespace dipper
