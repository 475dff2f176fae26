// Bootstrap support of the NJ tree of aligned sequences (`--bootstrap N`; no reference counterpart).  With --bionj the main tree
// and every replicate tree are BIONJ trees: the contexts carry the variant, everything here consumes merge logs only.
//
// The main tree is built exactly as without the option.  Then every rank runs its replicates r = rank, rank + world, .. with
// no collective: dpr_msa_resample (replicate alignment, on the device) -> dpr_dist_matrix -> dpr_nj_run -> dpr_split_support
// (host) into per-node counts.  One rank: the replicates reuse the main context and its NJ buffers.  Several ranks: each runs
// them on a rank-local second context on its own device (one rank, so no plan of the joined context -- and no collective --
// reaches the replicate loop).  One integer sum over the ranks combines the counts; rank 0 writes the labelled Newick.
// --bootstrap-metric tbe: dpr_transfer_support (device) in place of dpr_split_support, per-node sums of phi in place of the
// counts (one 64-bit sum over the ranks), transferLabels in place of supportLabels.
// --bootstrap-taxa FILE: dpr_transfer_taxa (device) per replicate -- in place of dpr_transfer_support with tbe, next to
// dpr_split_support with fbp -- adds to moved[tip] and pairs; one more 64-bit sum over the ranks; rank 0 writes FILE.  The report's
// tips are numbered in input order, so that call gets the trees with the tips renamed from slots to input indices (relabelledLog).
// --upgma / --wpgma (one rank): dpr_upgma_run in place of every dpr_nj_run; the first n - 2 entries of its log are a merge log of the
// same unrooted tree and go to the support functions unchanged, the whole log to writeNewickFromUpgma (the root carries no label).
#include "dipper_host.hpp"
#include "../csrc/merge_log.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <iostream>

namespace dipper {

// clade sizes, children and root pair of a log of dpr_nj_run / dpr_upgma_run (../csrc/merge_log.hpp)
static merge_log::Sizes cladeSizes(int64_t n, const std::vector<int32_t>& mx, const std::vector<int32_t>& my)
{
    merge_log::Sizes s;
    if (!merge_log::sizes_of<false>(n, mx.data(), my.data(), s)) die("ERROR: internal: the merge log names a slot that is not live");
    return s;
}

std::vector<int32_t> supportLabels(int64_t n, const std::vector<int32_t>& mx, const std::vector<int32_t>& my,
                                   const std::vector<int32_t>& counts, int64_t replicates)
{
    std::vector<int32_t> labels((size_t)std::max<int64_t>(n - 2, 1), -1);
    if (n <= 3 || replicates <= 0) return labels;
    const merge_log::Sizes t = cladeSizes(n, mx, my);
    for (int64_t k = 0; k < n - 2; ++k) {
        const int64_t s = t.size[(size_t)(n + k)];
        if (s >= 2 && s <= n - 2) labels[(size_t)k] = (int32_t)((200 * (int64_t)counts[(size_t)k] + replicates) / (2 * replicates));
    }
    return labels;
}

std::vector<int32_t> transferLabels(int64_t n, const std::vector<int32_t>& mx, const std::vector<int32_t>& my,
                                    const std::vector<int64_t>& phi_sum, int64_t replicates)
{
    std::vector<int32_t> labels((size_t)std::max<int64_t>(n - 2, 1), -1);
    if (n <= 3 || replicates <= 0) return labels;
    const merge_log::Sizes t = cladeSizes(n, mx, my);
    for (int64_t k = 0; k < n - 2; ++k) {
        const int64_t p = std::min<int64_t>(t.size[(size_t)(n + k)], n - t.size[(size_t)(n + k)]);
        if (p < 2) continue;
        const int64_t den = replicates * (p - 1), num = den - phi_sum[(size_t)k];
        labels[(size_t)k] = (int32_t)((200 * num + den) / (2 * den));
    }
    return labels;
}

// branches of the per-taxon report: internal nodes with p >= 2, the root's two children counting once
static int64_t taxaBranches(int64_t n, const std::vector<int32_t>& mx, const std::vector<int32_t>& my)
{
    if (n <= 3) return 0;
    const merge_log::Sizes t = cladeSizes(n, mx, my);
    auto p = [&](int64_t v) { return std::min<int64_t>(t.size[(size_t)v], n - t.size[(size_t)v]); };
    int64_t b = 0;
    for (int64_t k = 0; k < n - 2; ++k) b += p(n + k) >= 2;
    // (the root joins two complementary clades: both are branches exactly when both are internal nodes with p >= 2)
    if (t.root[0] >= n && t.root[1] >= n && p(t.root[0]) >= 2) --b;
    return b;
}

// The merge log of the same tree with tip `slot` renamed tipOf[slot]: the k-th merge joins the same two nodes into node n+k, so
// per-node results keep their index; only the slots (`at`, the slot map of the log being written, for the new names) differ.
static void relabelledLog(int64_t n, const std::vector<int32_t>& mx, const std::vector<int32_t>& my, const std::vector<int32_t>& tipOf,
                          std::vector<int32_t>& ox, std::vector<int32_t>& oy)
{
    std::vector<int32_t> real, at((size_t)n), slot_of((size_t)std::max<int64_t>(2 * n - 2, n));
    for (int64_t i = 0; i < n; ++i) at[(size_t)i] = slot_of[(size_t)i] = (int32_t)i;
    const bool ok = merge_log::replay<false>(n, n - 2, mx.data(), my.data(), real, [&](int64_t it, int32_t v, int32_t a, int32_t b) {
        const int32_t sa = slot_of[(size_t)(a < n ? tipOf[(size_t)a] : a)], sb = slot_of[(size_t)(b < n ? tipOf[(size_t)b] : b)];
        const int32_t lo = std::min(sa, sb), hi = std::max(sa, sb);
        ox[(size_t)it] = lo; oy[(size_t)it] = hi;
        merge_log::join_slots(at.data(), lo, hi, n - it, v);
        slot_of[(size_t)v] = lo; slot_of[(size_t)at[(size_t)hi]] = hi;      // (hi the last live slot: nothing moved)
    });
    if (!ok) die("ERROR: internal: the merge log names a slot that is not live");
}

// moved / pairs to six decimals, rounded half up, from integers only
static std::string indexText(int64_t moved, int64_t pairs)
{
    if (pairs <= 0) return "0.000000";
    const unsigned long long q = (unsigned long long)(((unsigned __int128)moved * 1000000u + (unsigned long long)(pairs / 2)) / (unsigned long long)pairs);
    char buf[48];
    std::snprintf(buf, sizeof(buf), "%llu.%06llu", q / 1000000ull, q % 1000000ull);
    return buf;
}

void bootstrapNeighbourJoiningTree(DeviceContext& dev, int numSequences, Param& params, const BootstrapOptions& bo,
                                   const uint64_t* packed4, int seqLen, std::vector<std::string>& name, std::ostream& output_)
{
    using Clock = std::chrono::steady_clock;
    auto ms = [](Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const int64_t n = numSequences, k = std::max<int64_t>(n - 2, 1);
    const RankInfo& ri = rankInfo();
    // the main tree (findNeighbourJoiningTree's run); its merge log is kept
    std::vector<int32_t> mx((size_t)k), my((size_t)k);
    std::vector<double> bx((size_t)k), by((size_t)k);
    double last = 0.0;
    // --upgma / --wpgma: every tree by dpr_upgma_run; the first n - 2 entries of its log are the unrooted tree everything below counts on
    const int linkage = upgmaOption();
    std::vector<int32_t> ux((size_t)(linkage >= 0 ? n - 1 : 0)), uy(ux.size()), urx(ux.size()), ury(ux.size());
    std::vector<double> uh(ux.size()), urh(ux.size());
    int64_t rescanned = 0;
    if (linkage >= 0) {
        const int64_t udone = dpr_upgma_run(dev.ctx, linkage, ux.data(), uy.data(), uh.data());
        if (udone < 0) gpuCheck((int)udone, "dpr_upgma_run");
        std::copy(ux.begin(), ux.begin() + (std::ptrdiff_t)(n - 2), mx.begin());
        std::copy(uy.begin(), uy.begin() + (std::ptrdiff_t)(n - 2), my.begin());
        int64_t stats[4] = { 0, 0, 0, 0 };
        dpr_get_upgma_stats(dev.ctx, stats);
        rescanned = stats[3];
    }
    const int64_t done = linkage >= 0 ? n - 2 : dpr_nj_run(dev.ctx, -1, mx.data(), my.data(), bx.data(), by.data(), &last);
    if (done < 0) gpuCheck((int)done, "dpr_nj_run");
    if (cliLog()) {
        double dist_ms = 0, nj_ms = 0;
        dpr_get_timing(dev.ctx, &dist_ms, &nj_ms);
        std::cerr << "  main tree: device distances " << dist_ms << " ms, NJ " << nj_ms << " ms\n";
    }

    const auto tb0 = Clock::now();
    std::vector<int32_t> counts((size_t)k, 0);
    std::vector<int64_t> phi_sum(bo.tbe || bo.taxa ? (size_t)k : 0, 0);
    std::vector<int64_t> moved(bo.taxa ? (size_t)n + 1 : 0, 0);      // by input index; [n]: the counted pairs
    // the report numbers the tips in input order: its trees go to dpr_transfer_taxa with the tips renamed from slots to that
    std::vector<int32_t> inputOf, imx, imy, irx, iry;     // (i..: the logs with the tips renamed to input indices)
    if (bo.taxa) {
        inputOf.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) inputOf[(size_t)bo.slotOfInput[(size_t)i]] = (int32_t)i;
        imx.resize((size_t)k); imy.resize((size_t)k); irx.resize((size_t)k); iry.resize((size_t)k);
        relabelledLog(n, mx, my, inputOf, imx, imy);
    }
    dpr_ctx* rctx = dev.ctx;
    auto fail = [&](int64_t r, const char* what, int rc) {
        die("ERROR: bootstrap replicate " + std::to_string(r) + ": " + what + " failed (" + std::to_string(rc) + "): " + dpr_last_error());
    };
    if (ri.world > 1 && ri.rank < bo.replicates) {
        // rank-local context: one rank, its own matrix (a second n x n on this device)
        dpr_ctx* c = nullptr;
        if (int rc = dpr_create(&c, ri.device)) fail(ri.rank, "dpr_create (rank-local context)", rc);
        rctx = c;
        if (bionjOption())
            if (int rc = dpr_ctx_set_nj_variant(rctx, 1)) fail(ri.rank, "dpr_ctx_set_nj_variant (rank-local context)", rc);
        if (int rc = dpr_set_msa(rctx, packed4, n, seqLen)) fail(ri.rank, "dpr_set_msa (rank-local context)", rc);
        filterSites(rctx, n, seqLen, false);      // (--site-coverage: the replicates resample the filtered alignment, as on one rank)
    }
    std::vector<int32_t> rx((size_t)k), ry((size_t)k);
    std::vector<double> rbx((size_t)k), rby((size_t)k);
    int64_t mine = 0;
    double mine_ms = 0;
    for (int64_t r = ri.rank; r < bo.replicates; r += ri.world) {
        const auto t0 = Clock::now();
        if (int rc = dpr_msa_resample(rctx, bo.seed, r)) fail(r, "dpr_msa_resample", rc);
        const auto t1 = Clock::now();
        if (int rc = dpr_dist_matrix(rctx, DPR_SRC_MSA, (int)params.distanceType, 0)) fail(r, "dpr_dist_matrix", rc);
        const auto t2 = Clock::now();
        double rlast = 0.0;
        int64_t rdone;
        if (linkage >= 0) {
            rdone = dpr_upgma_run(rctx, linkage, urx.data(), ury.data(), urh.data());
            if (rdone < 0) fail(r, "dpr_upgma_run", (int)rdone);
            std::copy(urx.begin(), urx.begin() + (std::ptrdiff_t)(n - 2), rx.begin());
            std::copy(ury.begin(), ury.begin() + (std::ptrdiff_t)(n - 2), ry.begin());
        } else {
            rdone = dpr_nj_run(rctx, -1, rx.data(), ry.data(), rbx.data(), rby.data(), &rlast);
            if (rdone < 0) fail(r, "dpr_nj_run", (int)rdone);
        }
        const auto t3 = Clock::now();
        if (bo.taxa) {
            relabelledLog(n, rx, ry, inputOf, irx, iry);
            if (int rc = dpr_transfer_taxa(rctx, n, imx.data(), imy.data(), irx.data(), iry.data(), bo.taxaCutoff, phi_sum.data(),
                                           moved.data(), moved.data() + n))
                fail(r, "dpr_transfer_taxa", rc);
            if (!bo.tbe)
                if (int rc = dpr_split_support(n, mx.data(), my.data(), rx.data(), ry.data(), counts.data())) fail(r, "dpr_split_support", rc);
        } else if (bo.tbe) {
            if (int rc = dpr_transfer_support(rctx, n, mx.data(), my.data(), rx.data(), ry.data(), phi_sum.data()))
                fail(r, "dpr_transfer_support", rc);
        } else if (int rc = dpr_split_support(n, mx.data(), my.data(), rx.data(), ry.data(), counts.data())) {
            fail(r, "dpr_split_support", rc);
        }
        const auto t4 = Clock::now();
        ++mine;
        mine_ms += ms(t0, t4);
        if (cliLog()) {
            double dist_ms = 0, nj_ms = 0;
            dpr_get_timing(rctx, &dist_ms, &nj_ms);
            std::cerr << "  replicate " << r << ": resample " << ms(t0, t1) << " ms, distances " << ms(t1, t2) << " ms (device "
                      << dist_ms << "), NJ " << ms(t2, t3) << " ms (device " << nj_ms << "), "
                      << (bo.tbe ? "transfer support " : "split count ") << (bo.taxa ? "and taxa " : "") << ms(t3, t4) << " ms\n";
        }
    }
    if (rctx != dev.ctx) dpr_destroy(rctx);
    else gpuCheck(dpr_msa_resample(dev.ctx, bo.seed, -1), "dpr_msa_resample");
    if (n > 2 && bo.tbe) gpuCheck(dpr_comm_sum_i64(dev.ctx, phi_sum.data(), n - 2), "dpr_comm_sum_i64");
    else if (n > 2) gpuCheck(dpr_comm_sum_i32(dev.ctx, counts.data(), n - 2), "dpr_comm_sum_i32");
    if (bo.taxa) gpuCheck(dpr_comm_sum_i64(dev.ctx, moved.data(), n + 1), "dpr_comm_sum_i64");
    const auto tb1 = Clock::now();

    const std::vector<int32_t> labels = bo.tbe ? transferLabels(n, mx, my, phi_sum, bo.replicates)
                                               : supportLabels(n, mx, my, counts, bo.replicates);
    if (linkage >= 0) {
        writeNewickFromUpgma(output_, name, ux, uy, uh, &labels);
        std::cerr << (linkage ? "WPGMA: " : "UPGMA: ") << n << " tips, root height " << uh[(size_t)(n - 2)] << ", " << rescanned << " rows rescanned\n";
    } else {
        writeNewickFromMerges(output_, name, mx, my, bx, by, last, &labels);
    }
    std::cerr << "Bootstrap: " << bo.replicates << " replicates (seed " << bo.seed << ") in " << (long long)ms(tb0, tb1) << " ms, "
              << (mine ? mine_ms / (double)mine : 0.0) << " ms per replicate, " << ri.world << " ranks"
              << (bo.tbe ? ", metric tbe (transfer bootstrap expectation)" : "") << "\n";
    if (bo.taxa) {
        const int64_t branches = taxaBranches(n, mx, my), pairs = moved[(size_t)n];
        char cut[16];
        std::snprintf(cut, sizeof(cut), "0.%03d", bo.taxaCutoff);
        std::ostream& os = *bo.taxa;
        os << "# dipper transfer index: replicates=" << bo.replicates << " seed=" << bo.seed << " cutoff=" << cut << " branches=" << branches
           << " pairs=" << pairs << "\ntaxon\tmoved\tindex\n";
        for (int64_t i = 0; i < n; ++i)
            os << name[(size_t)bo.slotOfInput[(size_t)i]] << "\t" << moved[(size_t)i] << "\t" << indexText(moved[(size_t)i], pairs) << "\n";
        os.flush();
        // the five taxa with the largest moved (ties: the earlier one in the input)
        std::vector<int64_t> top((size_t)n);
        for (int64_t t = 0; t < n; ++t) top[(size_t)t] = t;
        const size_t shown = (size_t)std::min<int64_t>(5, n);
        std::partial_sort(top.begin(), top.begin() + (std::ptrdiff_t)shown, top.end(), [&](int64_t a, int64_t b) {
            return moved[(size_t)a] != moved[(size_t)b] ? moved[(size_t)a] > moved[(size_t)b] : a < b;
        });
        std::cerr << "Transfer index: " << pairs << " of " << branches * bo.replicates << " (branch, replicate) pairs within cutoff " << cut
                  << "; most moved:";
        for (size_t i = 0; i < shown; ++i)
            std::cerr << " " << name[(size_t)bo.slotOfInput[(size_t)top[i]]] << " (" << moved[(size_t)top[i]] << ")";
        std::cerr << "\n";
    }
}

}  // namespace dipper
