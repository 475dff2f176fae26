// The reference's operator interface for the hot path over the C ABI (see dipper_host.hpp).
#include "dipper_host.hpp"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>

#include <sys/stat.h>

namespace dipper {

bool& bionjOption()
{
    static bool on = false;
    return on;
}

int& upgmaOption()
{
    static int linkage = -1;
    return linkage;
}

FitOption& fitOption()
{
    static FitOption o;
    return o;
}

// a double with 17 significant digits (round-trips); a NaN of either sign as `nan`
static std::string fitNumber(double v)
{
    if (v != v) return "nan";
    char buf[40];
    std::snprintf(buf, sizeof(buf), "%.17g", v);
    return buf;
}

void reportFit(DeviceContext& dev, const std::vector<std::string>& name, const std::vector<int32_t>& parent, const std::vector<double>& len)
{
    const FitOption& o = fitOption();
    const size_t n = name.size();
    double sums[16];
    std::vector<double> ss(n);
    std::vector<int64_t> pairs(n);
    int32_t worst[2] = { -1, -1 };
    gpuCheck(dpr_tree_fit(dev.ctx, (int64_t)n, (int64_t)parent.size(), parent.data(), len.data(), sums, ss.data(), pairs.data(), worst), "dpr_tree_fit");
    const std::string none = "-";
    std::cerr << "Fit: " << (long long)sums[0] << " pairs (" << (long long)sums[1] << " skipped), SS " << fitNumber(sums[7]) << ", rms " << fitNumber(sums[11])
              << ", relative rms " << fitNumber(sums[12]) << ", explained variance " << fitNumber(sums[13]) << ", cophenetic correlation "
              << fitNumber(sums[14]) << ", worst pair " << (worst[0] >= 0 ? name[(size_t)worst[0]] : none) << " / "
              << (worst[1] >= 0 ? name[(size_t)worst[1]] : none) << " (|d - p| = " << fitNumber(sums[10]) << ")\n";
    // per taxon: rms residual over its counted pairs, and that over the tree-wide rms
    const double zero = 0.0;
    std::vector<double> rms(n), rel(n);
    for (size_t t = 0; t < n; ++t) {
        rms[t] = pairs[t] > 0 ? std::sqrt(ss[t] / (double)pairs[t]) : zero / zero;
        rel[t] = rms[t] / sums[11];
    }
    std::vector<size_t> order(n);
    for (size_t t = 0; t < n; ++t) order[t] = t;
    // largest rms first, NaN last, ties by slot
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return rms[a] == rms[a] && (rms[b] != rms[b] || rms[a] > rms[b]); });
    std::cerr << "Fit: worst taxa";
    for (size_t k = 0; k < std::min<size_t>(5, n); ++k)
        std::cerr << (k ? ", " : " ") << name[order[k]] << " (rms " << fitNumber(rms[order[k]]) << ")";
    std::cerr << "\n";
    if (cliLog()) {
        double row_ms = 0, col_ms = 0;
        dpr_get_fit_timing(dev.ctx, &row_ms, &col_ms, nullptr);
        std::cerr << "  device: fit row pass " << row_ms << " ms, column pass " << col_ms << " ms\n";
    }
    if (!o.taxa || rankInfo().rank != 0) return;
    std::ostream& os = *o.taxa;
    os << "taxon\tpairs\tss\trms\trms_over_tree_rms\n";
    for (size_t i = 0; i < n; ++i) {
        const size_t t = o.slotOfInput.empty() ? i : (size_t)o.slotOfInput[i];
        os << name[t] << "\t" << pairs[t] << "\t" << fitNumber(ss[t]) << "\t" << fitNumber(rms[t]) << "\t" << fitNumber(rel[t]) << "\n";
    }
    os.flush();
}

SiteFilterOption& siteFilterOption()
{
    static SiteFilterOption o;
    return o;
}

int parseSiteCoverage(const std::string& v)
{
    // per mille from the text, as --bootstrap-taxa-cutoff: digits, at most one point, at most three places; the integer part is
    // zeros (or empty) with any places, or a one with places that are all zero
    const size_t dot = v.find('.');
    const std::string ip = v.substr(0, dot), fp = dot == std::string::npos ? "" : v.substr(dot + 1);
    if (v.empty() || (ip.empty() && fp.empty()) || fp.size() > 3 || ip.size() > 20) return 0;
    for (char ch : ip) if (!std::isdigit((unsigned char)ch)) return 0;
    for (char ch : fp) if (!std::isdigit((unsigned char)ch)) return 0;
    int pm = 0;
    for (size_t i = 0; i < 3; ++i) pm = 10 * pm + (i < fp.size() ? fp[i] - '0' : 0);
    size_t ones = 0, others = 0;
    for (size_t i = 0; i < ip.size(); ++i) {
        if (ip[i] == '1' && i + 1 == ip.size()) ++ones;
        else if (ip[i] != '0') ++others;
    }
    if (others) return 0;
    if (ones) return pm == 0 ? 1000 : 0;
    return pm;      // (0: out of range)
}

std::string siteCoverageText(int permille)
{
    if (permille >= 1000) return "1";
    char buf[16];
    std::snprintf(buf, sizeof(buf), "0.%03d", permille);
    std::string t = buf;
    while (t.back() == '0') t.pop_back();
    return t;
}

void filterSites(dpr_ctx* ctx, int64_t n, int64_t L, bool report)
{
    SiteFilterOption& o = siteFilterOption();
    if (!o.permille) return;
    const int64_t kept = dpr_msa_filter_sites(ctx, o.permille);
    if (kept < 0) {
        const std::string why = dpr_last_error();
        struct stat st;
        if (rankInfo().rank == 0 && !o.outputFile.empty() && stat(o.outputFile.c_str(), &st) == 0 && S_ISREG(st.st_mode))
            std::remove(o.outputFile.c_str());
        die("ERROR: --site-coverage " + o.text + ": " + why);
    }
    o.kept = kept;
    if (report) std::cerr << "Sites: kept " << kept << " of " << L << " (coverage >= " << o.text << " of " << n << " sequences)\n";
}

DeviceContext::DeviceContext(int device)
{
    gpuCheck(dpr_create(&ctx, device), "dpr_create");
    if (bionjOption()) gpuCheck(dpr_ctx_set_nj_variant(ctx, 1), "dpr_ctx_set_nj_variant");
    // one of several ranks (startRanks): join the others before any input reaches the device
    const RankInfo& ri = rankInfo();
    if (ri.world > 1) gpuCheck(dpr_comm_init_shared(ctx, ri.rank, ri.world, ri.region, DPR_COMM_SHARED_BYTES, ri.transport), "dpr_comm_init_shared");
}
DeviceContext::~DeviceContext() { if (ctx) dpr_destroy(ctx); }

void printRankSummary(dpr_ctx* ctx)
{
    if (rankInfo().world <= 1 || !ctx) return;
    int transport = 0, rank = 0, nranks = 1;
    int64_t coll = 0;
    dpr_comm_stats(ctx, &transport, &coll);
    dpr_comm_info(ctx, &rank, &nranks);
    static const char* const names[] = { "none", "rccl", "ipc", "local" };
    std::cerr << "Ranks: " << nranks << " (transport " << names[transport & 3] << ", " << coll << " device collectives)\n";
}

struct AsyncDeviceContext::Impl {
    std::thread th;
    DeviceContext* dev = nullptr;
    std::mutex mu;
    std::condition_variable cv;
    size_t reserve_n = 0;
    const uint64_t* msa_flat = nullptr;      // handed over by uploadMSA
    size_t msa_n = 0;
    int msa_len = 0;
    bool msa_done = false;
    bool closing = false;
    double create_ms = 0;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void lap(const char* what) const
    {
        if (cliLog()) std::fprintf(stderr, "  device thread: %s at %.1f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
};
double AsyncDeviceContext::createMs() const { return impl->create_ms; }
AsyncDeviceContext::AsyncDeviceContext(int device) : impl(new Impl)
{
    Impl* q = impl;
    impl->th = std::thread([q, device] {
        const auto tc0 = std::chrono::steady_clock::now();
        q->dev = new DeviceContext(device);
        q->create_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc0).count();
        q->lap("context created");
        // One thread, one dpr_* call at a time.  What main has handed over goes first, in this order: the NJ matrices (n is
        // known), the alignment (it is packed); then, once, the graph set-up of the HIP runtime (dpr_warm_graphs, 10-30 ms of
        // host work inside the runtime).  That warm-up used to run on a thread and a stream of its own; whatever ran beside it
        // queued behind the runtime's locks -- the upload took 20-60 ms there instead of 5, the distance kernel's launch
        // waited 25 -- and the private stream alone cost 9-16 ms.
        bool reserved = false, warmed = false;
        std::unique_lock<std::mutex> lk(q->mu);
        for (;;) {
            if (q->reserve_n != 0 && !reserved) {
                const size_t n = q->reserve_n;
                lk.unlock();
                (void)dpr_reserve_nj(q->dev->ctx, (int64_t)n);      // best effort: dpr_dist_matrix allocates what is missing
                q->lap("dpr_reserve_nj done");
                reserved = true;
                lk.lock();
            } else if (q->msa_flat && !q->msa_done) {
                lk.unlock();
                gpuCheck(dpr_set_msa(q->dev->ctx, q->msa_flat, (int64_t)q->msa_n, (int64_t)q->msa_len), "dpr_set_msa");
                q->lap("dpr_set_msa done");
                lk.lock();
                q->msa_done = true;
            } else if (!warmed) {
                lk.unlock();
                (void)dpr_warm_graphs(q->dev->ctx);
                q->lap("dpr_warm_graphs done");
                warmed = true;
                lk.lock();
            } else if (q->closing) {
                break;
            } else {
                q->cv.wait(lk);
            }
        }
    });
}
void AsyncDeviceContext::reserveNJ(size_t n)
{
    { std::lock_guard<std::mutex> lk(impl->mu); impl->reserve_n = n; }
    impl->cv.notify_all();
}
void AsyncDeviceContext::uploadMSA(const PackedSequences& packed)
{
    if (packed.numSequences < 2) return;      // (the caller's own checks end the run with their messages)
    { std::lock_guard<std::mutex> lk(impl->mu); impl->msa_flat = packed.flat.data(); impl->msa_n = packed.numSequences; impl->msa_len = packed.seqLen; }
    impl->cv.notify_all();
}
bool AsyncDeviceContext::msaUploaded() const { return impl->msa_done; }
DeviceContext& AsyncDeviceContext::get()
{
    { std::lock_guard<std::mutex> lk(impl->mu); impl->closing = true; }
    impl->cv.notify_all();
    if (impl->th.joinable()) impl->th.join();
    impl->lap("device thread joined");
    return *impl->dev;
}
AsyncDeviceContext::~AsyncDeviceContext()
{
    { std::lock_guard<std::mutex> lk(impl->mu); impl->closing = true; }
    impl->cv.notify_all();
    if (impl->th.joinable()) impl->th.join();
    delete impl->dev;
    delete impl;
}

void MSADeviceArrays::allocateDeviceArrays(DeviceContext& dev, const PackedSequences& packed, bool uploaded)
{
    numSequences = packed.numSequences;
    if (numSequences < 2) die("ERROR: need at least two sequences");
    seqLen = packed.seqLen;
    // (uploaded: AsyncDeviceContext::uploadMSA did it on the device thread)
    if (!uploaded) gpuCheck(dpr_set_msa(dev.ctx, packed.flat.data(), (int64_t)numSequences, (int64_t)seqLen), "dpr_set_msa");
    filterSites(dev.ctx, (int64_t)numSequences, (int64_t)seqLen, true);
}

void MashDeviceArrays::allocateDeviceArrays(DeviceContext& dev, const PackedSequences& packed)
{
    numSequences = packed.numSequences;
    if (numSequences < 2) die("ERROR: need at least two sequences");
    gpuCheck(dpr_set_reads(dev.ctx, packed.flat.data(), packed.off.data(), packed.lens.data(), (int64_t)numSequences), "dpr_set_reads");
}

void packAligned(const std::vector<std::string>& seqs, const std::vector<int>& ids, std::vector<uint64_t>& flat, int& seqLen)
{
    const size_t numSequences = seqs.size();
    // seqLen = length of the sequence in slot 0 (src/MSA.cu:19)
    size_t slot0 = 0;
    for (size_t i = 0; i < numSequences; ++i) if (ids[i] == 0) slot0 = i;
    seqLen = (int)seqs[slot0].size();
    const size_t W = ((size_t)seqLen + 15) / 16;
    flat.assign(numSequences * W, 0);
    unsigned nt = hostThreads(32);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t)
        pool.emplace_back([&, t] {
            std::vector<uint64_t> tmp;
            for (size_t i = t; i < numSequences; i += nt) {
                const std::string& s = seqs[i];
                tmp.assign((s.size() + 15) / 16 + 1, 0);
                dpr_pack4(s.data(), s.size(), tmp.data());
                // positions beyond a shorter sequence read as code 0 in the reference's flat buffer
                // only by accident (neighbouring data); here they are padded with the invalid code 4.
                uint64_t* dst = flat.data() + (size_t)ids[i] * W;
                const size_t have = (s.size() + 15) / 16;
                for (size_t w = 0; w < W; ++w) dst[w] = w < have ? tmp[w] : 0x4444444444444444ull;
                if (s.size() < (size_t)seqLen && have > 0 && have <= W) {
                    // tail of the last present word: mark the missing bases invalid
                    const size_t r = s.size() % 16;
                    if (r) dst[have - 1] |= 0x4444444444444444ull << (4 * r);
                }
            }
        });
    for (auto& th : pool) th.join();
}

// replaces the tbb::parallel_for packing loop (src/tree_generation.cu:352-362) + MSADeviceArrays::
// allocateDeviceArrays (src/MSA.cu:14-72)
void MSADeviceArrays::allocateDeviceArrays(DeviceContext& dev, const std::vector<std::string>& seqs,
                                           const std::vector<int>& ids)
{
    numSequences = seqs.size();
    if (numSequences < 2) die("ERROR: need at least two sequences");
    std::vector<uint64_t> flat;
    packAligned(seqs, ids, flat, seqLen);
    gpuCheck(dpr_set_msa(dev.ctx, flat.data(), (int64_t)numSequences, (int64_t)seqLen), "dpr_set_msa");
    filterSites(dev.ctx, (int64_t)numSequences, (int64_t)seqLen, true);
}

void MSADeviceArrays::allocateDeviceArraysProtein(DeviceContext& dev, const std::vector<std::string>& seqs, const std::vector<int>& ids)
{
    numSequences = seqs.size();
    if (numSequences < 2) die("ERROR: need at least two sequences");
    size_t slot0 = 0;
    for (size_t i = 0; i < numSequences; ++i) if (ids[i] == 0) slot0 = i;
    seqLen = (int)seqs[slot0].size();
    if (seqLen < 1) die("ERROR: the first sequence of the alignment is empty");
    const size_t L = (size_t)seqLen;
    std::vector<uint8_t> codes(numSequences * L, (uint8_t)255);
    const unsigned nt = hostThreads(32);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t)
        pool.emplace_back([&, t] {
            for (size_t i = t; i < numSequences; i += nt)
                dpr_pack_aa(seqs[i].data(), std::min(seqs[i].size(), L), codes.data() + (size_t)ids[i] * L);
        });
    for (auto& th : pool) th.join();
    gpuCheck(dpr_set_msa_aa(dev.ctx, codes.data(), (int64_t)numSequences, (int64_t)seqLen), "dpr_set_msa_aa");
    filterSites(dev.ctx, (int64_t)numSequences, (int64_t)seqLen, true);
}

void NJDeviceArrays::getDismatrix(DeviceContext& dev, int numSequences, Param& params, MatrixReader* matrixReader)
{
    d_numSequences = numSequences;
    if (params.in == "d") {
        gpuCheck(dpr_set_matrix_lower(dev.ctx, matrixReader->lower.data(), numSequences), "dpr_set_matrix_lower");
        gpuCheck(dpr_dist_matrix(dev.ctx, DPR_SRC_MATRIX, 0, 0), "dpr_dist_matrix");
    } else if (params.in == "m") {
        gpuCheck(dpr_dist_matrix(dev.ctx, DPR_SRC_MSA, (int)params.distanceType, 0), "dpr_dist_matrix");
    } else {
        gpuCheck(dpr_dist_matrix(dev.ctx, DPR_SRC_MASH, 0, (int)params.kmerSize), "dpr_dist_matrix");
    }
    if (rankInfo().world > 1) {
        char plan[256] = "";
        dpr_get_nj_multi_info(dev.ctx, plan, (int)sizeof plan);
        std::cerr << "NJ over " << rankInfo().world << " ranks: " << plan << "\n";
    }
}

void NJDeviceArrays::findNeighbourJoiningTree(DeviceContext& dev, std::vector<std::string>& name, std::ostream& output_, Param* params,
                                              MatrixReader* matrixReader)
{
    const int N = d_numSequences;
    std::vector<int32_t> mx((size_t)std::max(N - 2, 1)), my((size_t)std::max(N - 2, 1));
    std::vector<double> bx((size_t)std::max(N - 2, 1)), by((size_t)std::max(N - 2, 1));
    double last = 0.0;
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t done = dpr_nj_run(dev.ctx, -1, mx.data(), my.data(), bx.data(), by.data(), &last);
    if (done < 0) gpuCheck((int)done, "dpr_nj_run");
    const auto t1 = std::chrono::steady_clock::now();
    writeNewickFromMerges(output_, name, mx, my, bx, by, last);
    if (cliLog()) {
        double dist_ms = 0, nj_ms = 0;
        dpr_get_timing(dev.ctx, &dist_ms, &nj_ms);
        std::cerr << "  device: distances " << dist_ms << " ms, NJ " << nj_ms << " ms; dpr_nj_run call "
                  << std::chrono::duration<double, std::milli>(t1 - t0).count() << " ms; Newick text "
                  << std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count() << " ms\n";
    }
    if (fitOption().on && params) {
        output_.flush();
        // the NJ run consumed the matrix: the fit reads a fresh one.  No NJ run follows, so it is built under the streaming plan: in slot
        // space, where both passes of the fit read coalesced, and without the pruned plan's first epoch
        gpuCheck(dpr_ctx_set_nj_mode(dev.ctx, 0), "dpr_ctx_set_nj_mode");
        getDismatrix(dev, N, *params, matrixReader);
        std::vector<int32_t> parent((size_t)(2 * N - 1));
        std::vector<double> len((size_t)(2 * N - 1));
        int64_t m = 0;
        gpuCheck(dpr_tree_from_nj(N, mx.data(), my.data(), bx.data(), by.data(), last, parent.data(), len.data(), &m), "dpr_tree_from_nj");
        reportFit(dev, name, parent, len);
    }
}

void NJDeviceArrays::findUpgmaTree(DeviceContext& dev, std::vector<std::string>& name, std::ostream& output_, int linkage)
{
    const int N = d_numSequences;
    std::vector<int32_t> mx((size_t)(N - 1)), my((size_t)(N - 1));
    std::vector<double> h((size_t)(N - 1));
    const int64_t done = dpr_upgma_run(dev.ctx, linkage, mx.data(), my.data(), h.data());
    if (done < 0) gpuCheck((int)done, "dpr_upgma_run");
    writeNewickFromUpgma(output_, name, mx, my, h);
    int64_t stats[4] = { 0, 0, 0, 0 };
    dpr_get_upgma_stats(dev.ctx, stats);
    std::cerr << (linkage ? "WPGMA: " : "UPGMA: ") << N << " tips, root height " << h[(size_t)(N - 2)] << ", " << stats[3] << " rows rescanned\n";
    if (cliLog()) {
        double loop_ms = 0;
        dpr_get_upgma_timing(dev.ctx, &loop_ms);
        std::cerr << "  device: " << (linkage ? "WPGMA" : "UPGMA") << " loop " << loop_ms << " ms, " << stats[2] << " launches\n";
    }
    if (fitOption().on) {      // (dpr_upgma_run works on a copy: the matrix is still fresh)
        output_.flush();
        std::vector<int32_t> parent((size_t)(2 * N - 1));
        std::vector<double> len((size_t)(2 * N - 1));
        int64_t m = 0;
        gpuCheck(dpr_tree_from_upgma(N, mx.data(), my.data(), h.data(), parent.data(), len.data(), &m), "dpr_tree_from_upgma");
        reportFit(dev, name, parent, len);
    }
}

void NJDeviceArrays::findRefinedTree(DeviceContext& dev, Param& params, MatrixReader* matrixReader, std::vector<std::string>& name,
                                     std::ostream& output_, int rounds, bool spr)
{
    const int N = d_numSequences;
    std::vector<int32_t> mx((size_t)std::max(N - 2, 1)), my((size_t)std::max(N - 2, 1));
    const int64_t done = dpr_nj_run(dev.ctx, -1, mx.data(), my.data(), nullptr, nullptr, nullptr);
    if (done < 0) gpuCheck((int)done, "dpr_nj_run");
    getDismatrix(dev, N, params, matrixReader);      // (the NJ run consumed the matrix: the search reads a fresh one)
    std::vector<int32_t> kids((size_t)(2 * std::max(N - 2, 1)));
    std::vector<double> len((size_t)(2 * N - 2)), L((size_t)rounds + 1, 0.0);
    int32_t top = 0;
    int64_t stats[6] = { 0, 0, 0, 0, 0, 0 };
    if (spr) gpuCheck(dpr_bme_spr(dev.ctx, N, mx.data(), my.data(), rounds, kids.data(), &top, len.data(), L.data(), stats), "dpr_bme_spr");
    else gpuCheck(dpr_bme_nni(dev.ctx, N, mx.data(), my.data(), rounds, kids.data(), &top, len.data(), L.data(), stats), "dpr_bme_nni");
    writeNewickFromKids(output_, name, kids, top, len);
    if (spr)
        std::cerr << "BME SPR: L " << L[0] << " -> " << L[(size_t)stats[0]] << ", " << stats[1] << " moves (" << stats[4] << " beyond NNI, longest "
                  << stats[5] << "), " << stats[0] << " rounds, " << stats[2] << " fallbacks\n";
    else
        std::cerr << "BME NNI: L " << L[0] << " -> " << L[(size_t)stats[0]] << ", " << stats[1] << " moves, " << stats[0] << " rounds, " << stats[2]
                  << " fallbacks\n";
    if (cliLog()) {
        double table_ms = 0, select_ms = 0, scan_ms = 0;
        dpr_get_bme_timing(dev.ctx, &table_ms, &select_ms);
        std::cerr << "  device: BME tables " << table_ms << " ms, lengths and gains " << select_ms << " ms";
        if (spr) {
            dpr_get_bme_spr_timing(dev.ctx, &scan_ms);
            std::cerr << ", SPR scans " << scan_ms << " ms";
        }
        std::cerr << "\n";
    }
    if (fitOption().on) {      // (the search read the fresh matrix and left it so)
        output_.flush();
        std::vector<int32_t> parent((size_t)(2 * N - 1));
        std::vector<double> flen((size_t)(2 * N - 1));
        int64_t m = 0;
        gpuCheck(dpr_tree_from_kids(N, kids.data(), top, len.data(), parent.data(), flen.data(), &m), "dpr_tree_from_kids");
        reportFit(dev, name, parent, flen);
    }
}

void packUnaligned(const std::vector<std::string>& seqs, const std::vector<int>& ids, std::vector<uint64_t>& flat,
                   std::vector<uint64_t>& off, std::vector<uint64_t>& lens)
{
    const size_t numSequences = seqs.size();
    lens.assign(numSequences, 0); off.assign(numSequences, 0);
    std::vector<uint64_t> nw(numSequences);
    for (size_t i = 0; i < numSequences; ++i) {
        lens[(size_t)ids[i]] = seqs[i].size();
        nw[(size_t)ids[i]] = (seqs[i].size() + 31) / 32;
    }
    uint64_t total = 0;
    for (size_t s = 0; s < numSequences; ++s) { off[s] = total; total += nw[s]; }  // exclusive scan (src/mash.cu:109-119)
    flat.assign(total + 1, 0);
    unsigned nt = hostThreads(32);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t)
        pool.emplace_back([&, t] {
            for (size_t i = t; i < numSequences; i += nt)
                if (!seqs[i].empty()) dpr_pack2(seqs[i].data(), seqs[i].size(), flat.data() + off[(size_t)ids[i]]);
        });
    for (auto& th : pool) th.join();
}

void MashDeviceArrays::allocateDeviceArrays(DeviceContext& dev, const std::vector<std::string>& seqs,
                                            const std::vector<int>& ids)
{
    numSequences = seqs.size();
    if (numSequences < 2) die("ERROR: need at least two sequences");
    std::vector<uint64_t> lens, off, flat;
    packUnaligned(seqs, ids, flat, off, lens);
    gpuCheck(dpr_set_reads(dev.ctx, flat.data(), off.data(), lens.data(), (int64_t)numSequences), "dpr_set_reads");
}

void MashDeviceArrays::sketchConstructionOnGpu(DeviceContext& dev, Param& params)
{
    gpuCheck(dpr_sketch(dev.ctx, (int)params.kmerSize, (int)params.sketchSize, nullptr), "dpr_sketch");
}

// ---- Newick import ---------------------------------------------------------------------------------
Tree::Tree(const std::string& newick_in, size_t totalLeaves)
{
    // (the text without line breaks; copied only if it has any.  500 000 tips: 17 MB, a million nodes -- the vector is sized once, a
    //  node's children get room for two, nodes are moved into place)
    std::string stripped;
    if (newick_in.find_first_of("\n\r") != std::string::npos) {
        stripped.reserve(newick_in.size());
        for (char c : newick_in) if (c != '\n' && c != '\r') stripped.push_back(c);
    }
    const std::string& s = stripped.empty() ? newick_in : stripped;
    nodes.reserve(2 * totalLeaves + 2);
    size_t nextInternal = totalLeaves, nextLeaf = 0;
    std::vector<int> stack;
    int last = -1;  // node whose label / length is being read
    auto parse_len = [&](size_t& i) {
        std::string num;
        size_t j = i + 1;
        while (j < s.size() && s[j] != ',' && s[j] != ')' && s[j] != '(' && s[j] != ';') {
            const char c = s[j];
            if (std::isdigit((unsigned char)c) || c == '.' || c == 'e' || c == 'E' || c == '-' || c == '+') num.push_back(c);
            ++j;
        }
        i = j - 1;
        return num.empty() ? 0.0 : (double)std::strtof(num.c_str(), nullptr);
    };
    for (size_t i = 0; i < s.size(); ++i) {
        const char c = s[i];
        if (c == '(') {
            Node nd;
            nd.idx = (int)nextInternal++;
            nd.name = "node_" + std::to_string(nd.idx);
            nd.parent = stack.empty() ? -1 : stack.back();
            nd.children.reserve(2);
            const int par = nd.parent;
            nodes.push_back(std::move(nd));
            const int id = (int)nodes.size() - 1;
            if (par >= 0) nodes[(size_t)par].children.push_back(id); else root = id;
            stack.push_back(id);
            last = -1;
        } else if (c == ')') {
            if (stack.empty()) die("ERROR: incorrect Newick format!");
            last = stack.back();
            stack.pop_back();
            // an internal label / support value after ')' is ignored, as in the reference
            size_t j = i + 1;
            while (j < s.size() && s[j] != ':' && s[j] != ',' && s[j] != ')' && s[j] != ';') ++j;
            i = j - 1;
        } else if (c == ',') {
            last = -1;
        } else if (c == ':') {
            const double v = parse_len(i);
            if (last >= 0) nodes[(size_t)last].bl = v;
        } else if (c == ';') {
            break;
        } else if (std::isspace((unsigned char)c)) {
            continue;
        } else {
            // leaf label (quoted labels keep their inner text)
            std::string name;
            size_t j = i;
            if (c == '\'') {
                ++j;
                while (j < s.size() && s[j] != '\'') name.push_back(s[j++]);
                ++j;
            } else {
                while (j < s.size() && s[j] != ':' && s[j] != ',' && s[j] != ')' && s[j] != '(' && s[j] != ';') name.push_back(s[j++]);
            }
            i = j - 1;
            if (stack.empty()) die("ERROR: incorrect Newick format!");
            Node nd;
            nd.idx = (int)nextLeaf++;
            nd.name = std::move(name);
            nd.parent = stack.back();
            const int par = nd.parent;
            nodes.push_back(std::move(nd));
            last = (int)nodes.size() - 1;
            nodes[(size_t)par].children.push_back(last);
        }
    }
    if (!stack.empty()) die("ERROR: incorrect Newick format!");
    if (root < 0) die("ERROR: Tree found empty!");
    nodes[(size_t)root].bl = 0;
    m_numLeaves = nextLeaf;
}

int Tree::findLeaf(const std::string& name) const
{
    for (size_t i = 0; i < nodes.size(); ++i)
        if (nodes[i].children.empty() && nodes[i].name == name) return (int)i;
    return -1;
}

// ---- placement ----------------------------------------------------------------------------------------
void KPlacementDeviceArrays::allocateDeviceArrays(size_t num, int backbone)
{
    numSequences = (int)num;
    backboneSize = backbone;
    bd = 2;
    h_head.assign(num * 2, -1);
    h_e.assign(num * 8, -1);
    h_nxt.assign(num * 8, -1);
    h_belong.assign(num * 8, -1);
    h_len.assign(num * 8, 2.0);
}

void KPlacementDeviceArrays::initializeDeviceArrays(const Tree& t)
{
    // post-order DFS; per tree edge two directed slots (child->parent, parent->child), each pushed
    // at the front of its source's list (src/placement_close_k.cu:160-183)
    size_t edgeCount = 0;
    struct Frame { int node; size_t next; };
    std::vector<Frame> st;
    st.push_back(Frame{ t.root, 0 });
    while (!st.empty()) {
        Frame& f = st.back();
        const Node& nd = t.nodes[(size_t)f.node];
        if (f.next < nd.children.size()) {
            const int c = nd.children[f.next++];
            st.push_back(Frame{ c, 0 });
            continue;
        }
        if (nd.parent >= 0) {
            const int x = nd.idx, y = t.nodes[(size_t)nd.parent].idx;
            if (edgeCount + 2 > h_e.size()) die("ERROR: backbone tree does not fit the allocated arrays");
            h_e[edgeCount] = y; h_len[edgeCount] = nd.bl; h_belong[edgeCount] = x;
            h_nxt[edgeCount] = h_head[(size_t)x]; h_head[(size_t)x] = (int32_t)edgeCount; edgeCount++;
            h_e[edgeCount] = x; h_len[edgeCount] = nd.bl; h_belong[edgeCount] = y;
            h_nxt[edgeCount] = h_head[(size_t)y]; h_head[(size_t)y] = (int32_t)edgeCount; edgeCount++;
        }
        st.pop_back();
    }
}

static int sourceOf(const Param& params)
{
    return params.in == "r" ? DPR_SRC_MASH : (params.in == "m" ? DPR_SRC_MSA : DPR_SRC_MATRIX);
}

// the reference's two timing lines (src/placement_close_k.cu:852-853,985-986).  With Mash input the distance rows of the
// next batch are computed beside the tree kernels: the first line is then the time the tree kernels waited for rows
// (the two lines still add up to the run) and a third line gives the batches' own, overlapped duration.
static void printPlaceTiming(DeviceContext& dev)
{
    double dist_ms = 0, tree_ms = 0, busy_ms = 0;
    int overlapped = 0;
    dpr_get_place_timing(dev.ctx, &dist_ms, &tree_ms);
    dpr_get_place_overlap(dev.ctx, &overlapped, &busy_ms);
    std::cerr << "Distance Operation Time " << (long long)dist_ms << " ms\n";
    std::cerr << "Tree Operation Time " << (long long)tree_ms << " ms\n";
    if (overlapped) {
        int64_t batches = 0, beside = 0;
        dpr_get_place_policy(dev.ctx, &batches, &beside);
        std::cerr << "Distance batches overlapped with tree operations: " << beside << " of " << batches << ", " << (long long)busy_ms << " ms in flight\n";
    }
}

void KPlacementDeviceArrays::findPlacementTree(DeviceContext& dev, Param& params)
{
    if (exact) {
        gpuCheck(dpr_place_exact_run(dev.ctx, sourceOf(params), (int)params.distanceType, (int)params.kmerSize, numSequences,
                                     h_head.data(), h_e.data(), h_nxt.data(), h_belong.data(), h_len.data()),
                 "dpr_place_exact_run");
        double dist_ms = 0, tree_ms = 0;
        dpr_get_timing(dev.ctx, &dist_ms, &tree_ms);    // (the exact mode's distance rows are produced inside its per-tip loop)
        std::cerr << "Distance + Tree Operation Time " << (long long)tree_ms << " ms\n";
        return;
    }
    gpuCheck(dpr_place_run(dev.ctx, sourceOf(params), (int)params.distanceType, (int)params.kmerSize, 2, numSequences,
                           h_head.data(), h_e.data(), h_nxt.data(), h_belong.data(), h_len.data()), "dpr_place_run");
    printPlaceTiming(dev);
}

void KPlacementDeviceArrays::addQuery(DeviceContext& dev, Param& params)
{
    gpuCheck(dpr_place_run(dev.ctx, sourceOf(params), (int)params.distanceType, (int)params.kmerSize, backboneSize,
                           numSequences, h_head.data(), h_e.data(), h_nxt.data(), h_belong.data(), h_len.data()),
             "dpr_place_run");
    printPlaceTiming(dev);
}

void KPlacementDeviceArrays::placeFixed(DeviceContext& dev, Param& params, const BootstrapOptions& bo, std::vector<std::vector<PlacementRow>>& rows)
{
    const size_t nq = (size_t)(numSequences - backboneSize);
    gpuCheck(dpr_place_fixed_set(dev.ctx, backboneSize, numSequences, h_head.data(), h_e.data(), h_nxt.data(), h_belong.data(), h_len.data()),
             "dpr_place_fixed_set");
    std::vector<int32_t> slot(nq);
    std::vector<double> frac(nq), add(nq);
    double dist_ms = 0, scan_ms = 0;
    auto run = [&]() {
        gpuCheck(dpr_place_fixed_run(dev.ctx, sourceOf(params), (int)params.distanceType, (int)params.kmerSize, slot.data(), frac.data(), add.data()),
                 "dpr_place_fixed_run");
        double d = 0, s = 0;
        dpr_get_place_fixed_timing(dev.ctx, &d, &s);
        dist_ms += d; scan_ms += s;
    };
    // frac is measured from belong[slot]: the child end for the even slot of an edge, the parent end for the odd one
    auto row_of = [&](size_t q) {
        const int32_t s = slot[q];
        if (s < 0) die("ERROR: a query has no placement");
        return PlacementRow{ s >> 1, 0, (s & 1) ? h_len[(size_t)s] - frac[q] : frac[q], add[q] };
    };
    // a placement whose lengths are not finite (a query at +inf from every tip of a backbone: JC at p >= 0.75) cannot be written
    // as JSON and says nothing: it is left out -- the query as a whole when it is the placement from the uploaded alignment, the
    // replicate's vote for that query otherwise
    auto finite = [](const PlacementRow& r) { return std::isfinite(r.pendant) && std::isfinite(r.distal); };
    run();
    rows.assign(nq, {});
    for (size_t q = 0; q < nq; ++q) {
        const PlacementRow r = row_of(q);
        if (finite(r)) rows[q].push_back(r);
    }
    std::cerr << "Distance Operation Time " << (long long)dist_ms << " ms\n";
    std::cerr << "Placement Scan Time " << (long long)scan_ms << " ms\n";
    if (bo.replicates <= 0) { for (auto& r : rows) if (!r.empty()) r[0].count = 1; return; }
    dist_ms = scan_ms = 0;
    for (int64_t r = 0; r < bo.replicates; ++r) {
        gpuCheck(dpr_msa_resample(dev.ctx, bo.seed, r), "dpr_msa_resample");
        run();
        for (size_t q = 0; q < nq; ++q) {
            const PlacementRow now = row_of(q);
            std::vector<PlacementRow>& v = rows[q];
            if (v.empty() || !finite(now)) continue;
            size_t k = 0;
            while (k < v.size() && v[k].edge != now.edge) ++k;
            if (k == v.size()) v.push_back(now);      // (replicates ascend: the lengths of the first one that chose the edge stay)
            ++v[k].count;
        }
    }
    gpuCheck(dpr_msa_resample(dev.ctx, bo.seed, -1), "dpr_msa_resample");
    std::cerr << "Bootstrap placements: " << bo.replicates << " replicates, distances " << (long long)dist_ms << " ms, scans " << (long long)scan_ms << " ms\n";
    for (auto& v : rows) {
        if (v.empty()) continue;
        const int32_t main_edge = v[0].edge;
        std::sort(v.begin(), v.end(), [main_edge](const PlacementRow& a, const PlacementRow& b) {
            if (a.count != b.count) return a.count > b.count;
            if ((a.edge == main_edge) != (b.edge == main_edge)) return a.edge == main_edge;
            return a.edge < b.edge;
        });
    }
}

void KPlacementDeviceArraysDC::allocateDeviceArraysDC(size_t num, size_t totalNum)
{
    allocateDeviceArrays(totalNum);          // arrays sized by the total tip count, node ids start there
    backboneSize = (int)num;
    totalNumSequences = (int)totalNum;
    clusterID.assign(totalNum, -1);
}

void KPlacementDeviceArraysDC::findTreeDC(DeviceContext& dev, Param& params)
{
    gpuCheck(dpr_dc_run(dev.ctx, sourceOf(params), (int)params.distanceType, (int)params.kmerSize, totalNumSequences,
                        backboneSize, 0, h_head.data(), h_e.data(), h_nxt.data(), h_belong.data(), h_len.data(),
                        clusterID.data()), "dpr_dc_run");
    int64_t counts[5] = { 0, 0, 0, 0, 0 };
    double ms[3] = { 0, 0, 0 };
    dpr_get_dc_stats(dev.ctx, counts, ms);
    std::cerr << "Finished backbone construction in: " << (long long)ms[0] << " ms\n";
    std::cerr << "Finished clustering in: " << (long long)ms[1] << " ms\n";
    std::cerr << "Finished cluster trees in: " << (long long)ms[2] << " ms (" << counts[0] << " clusters, largest "
              << counts[1] << ")\n";
}

// printTree (src/placement_close_k.cu:568-643), iterative: root = node numSequences+bd-2, children in
// adjacency-list order, the edge back to the parent skipped; a node with a single adjacency entry is a leaf.
void KPlacementDeviceArrays::printTree(const std::vector<std::string>& name, std::ostream& output_)
{
    // (a node's adjacency entries other than the one it was entered through, gathered once into one array: no allocation per node)
    struct Frame { int node, from; size_t first, count, next; };
    std::vector<int> pos;
    pos.reserve((size_t)numSequences * 4);
    auto make = [&](int node, int from) {
        Frame f{ node, from, pos.size(), 0, 0 };
        for (int i = h_head[(size_t)node]; i != -1; i = h_nxt[(size_t)i])
            if (h_e[(size_t)i] != from) pos.push_back(i);
        f.count = pos.size() - f.first;
        return f;
    };
    auto is_internal = [&](int node) { return h_nxt[(size_t)h_head[(size_t)node]] != -1; };
    const int root = numSequences + bd - 2;
    std::vector<Frame> st;
    if (!is_internal(root)) { output_ << name[(size_t)root] << ";\n"; return; }
    TextBuf out;
    out.s.reserve((size_t)numSequences * 40);
    out.put('(');
    st.push_back(make(root, -1));
    while (!st.empty()) {
        Frame& f = st.back();
        if (f.next == f.count) {
            pos.resize(f.first);             // (frames end in the order they began: the array is a stack)
            st.pop_back();
            if (st.empty()) break;
            Frame& up = st.back();
            out.put(':'); out.putLength(h_len[(size_t)pos[up.first + up.next - 1]]); out.put(up.next == up.count ? ')' : ',');
            continue;
        }
        const int slot = pos[f.first + f.next++];
        const int child = h_e[(size_t)slot];
        if (is_internal(child)) {
            out.put('(');
            const int parent = f.node;       // (push_back may move the frames)
            st.push_back(make(child, parent));
        } else {
            out.put(name[(size_t)child]); out.put(':'); out.putLength(h_len[(size_t)slot]); out.put(f.next == f.count ? ')' : ',');
        }
    }
    out.put(";\n");
    output_.write(out.s.data(), (std::streamsize)out.s.size());
}

}  // namespace dipper
