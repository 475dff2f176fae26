// What a `dipper` command line means: parsed, checked and held in one struct (options.cpp).  A new option's rules go into
// parseOptions, in the place the order of the messages gives them (tests/golden/cli_usage_matrix.tsv).
#pragma once
#include "dipper_host.hpp"

namespace dipper {

extern const char* const kHelp;

struct Options {
    bool help = false;
    // a --dump-* developer aid (devaids.cpp), named as its option is, and that option's value: nothing is checked then
    std::string aid, aidArg;
    Param params;
    BootstrapOptions boot;
    RankOptions ranks;
    std::string inputFile, outputFile, treeFile, bootTaxaFile, fitTaxaFile, clustersFile;
    std::string algo = "0";      // -m
    bool exact_mode = false, add = false, jplace = false, protein = false, bionj = false, spr = false, fit = false;
    int nni = -1;                // rounds of --nni / --spr, -1 = no refinement
    int upgma = -1;              // the linkage: 0 --upgma, 1 --wpgma, -1 = NJ
    int sitePermille = 0;        // --site-coverage / --complete-deletion, 0 = off
    bool pairs = false;          // -o p: the pairs within --within and, with --clusters, the clusters they form
    double within = 0;           // --within T, a finite number >= 0 ...
    std::string withinText;      // ... and T as it was given (the reports name it so)
    bool nearest = false;        // -o n: the --nearest K nearest neighbours of every sequence
    int nearestK = 0;
    bool mst = false;            // -o s: the minimum spanning tree of the distances and, with --dendrogram, the single-linkage tree
    std::string dendrogramFile;
    std::string siteText;
    long long seed = 1;
    int device = 0;
    bool multi = false;          // several ranks
    // the option given that builds its tree where conventional NJ does, as checkedMode names it ("--bionj needs conventional NJ");
    // of several the first of --bootstrap, --bionj, --nni / --spr, --upgma / --wpgma, --fit
    std::string njOnly;
};

// Ends the process only through usageError (the message in red, the help, exit 1); sets no global, opens no file.
Options parseOptions(int argc, char** argv);
// The four process-wide option singletons (bionjOption, upgmaOption, fitOption, siteFilterOption), set once
void applyOptions(const Options& o);

// Mode selection of the reference (src/tree_generation.cu:377,422,450) for n sequences: 1 = placement, 3 = divide-and-conquer,
// 2 = conventional NJ.  checkedMode: the same, once the size of the input is known -- it ends the run when an option that was
// given cannot be had in that mode.
int pickMode(const Options& o, long long n);
int checkedMode(const Options& o, long long n);

int runDeveloperAid(const Options& o);      // devaids.cpp; the exit status

}  // namespace dipper
