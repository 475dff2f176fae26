// Which batches of distance rows a k-closest placement run produces BESIDE the previous batch's tree kernels (on a second,
// low-priority stream) and which on the main stream right before their own tips.  Host-only: nothing of HIP in here, so the rule
// runs without a device (dpr_place_policy_run, tests/test_place_policy.py).  place_range (ctx_place.hip) asks it once per batch.
//
// Why there is a rule.  The tree kernels of a batch are latency-bound and occupy a few workgroups; the pair kernels of the next
// batch fill the rest of the chip.  Overlap pays while a batch's distance part is the SHORTER one: it disappears behind the tree
// kernels (100 000 unaligned tips from scratch: 3.2 -> 2.5 s).  Where it is the longer one nothing can hide it and sharing the
// chip slows both sides: adding 50 000 queries to a 500 000-tip backbone, every batch is 5 x 10^8 pairs (~100 ms alone) against
// ~50 ms of tree kernels; overlapped, the pair kernel ran at half its rate and the update kernel 5.6 x slower
// (profiles/r3/kernel_stats_add_mash_500k_plus_50k.csv): 9.2 s where back to back is 7.6 s.
//   * Mash input only: with aligned input the distance part is 4 % of the run and the contention costs more than it hides
//     (1.63 -> 1.82 s at 100 000 tips); the packed triangle is read in place.  Not for ranks on the window transport of
//     dpr_comm_init_shared either: its all-gather is synchronous with the host, nothing would overlap.
//   * Several ranks: every rank must take the same decisions (a batch's all-gather is enqueued on the stream the decision
//     picks), and a rank's share of a batch is 1 / G of the pairs, i.e. the short side: every batch beside.
//   * While the tree kernels are the one-tip launch pairs (a 780-block scan and a one-workgroup update every 15 us; tips below
//     place_multi_min(), 150 000) EVERY batch goes beside them, longer than the tree part or not: 100 000 unaligned tips
//     2.18 -> 1.72 s (mean branch 2e-5), 2.30 -> 2.14 s (1e-3).
//   * The four-tip launch pairs above that: their scan fills the chip for 54 us of every ~120, so the pair kernel beside it gets
//     half a chip (--add through Mash, every batch beside: 6.8 s against 4.0 s; the 1 024-thread update workgroup needs an empty
//     CU and waits 0.5 ms for one).  There batch k + 1 goes beside batch k's tree kernels iff its predicted time alone -- pairs /
//     the rate measured on this run's batches that were produced alone, 4.5 G pairs/s until there is one of >= 5 x 10^7 pairs --
//     is below the tree time of the latest finished batch.  Tree kernels that shared the chip ran ~1.3 x slower at 100 000
//     tips: such a batch's time is deflated by 1.4 before it stands for "the tree part alone" (the tree part grows with the
//     tree, so the latest batch is a better estimate than batch 0's clean one).  Before any tree time exists (batch 0) the
//     successor goes beside only if its distance part is tiny (< 1 ms).  Measured (profiles/r4/place_policy_*.jsonl): --add
//     500 000 + 50 000 through Mash 8.87 s (every batch beside) -> 6.56 s (none); 100 000 tips from scratch 3.07 s (none) /
//     2.52 s (every batch) / 2.5x s (policy).
// The timed rule is the only case that reads timings: the host then waits for batch k - 1 before it decides about batch k + 1
// (enqueueing is ~10 x faster than the tree kernels execute, so the device does not starve); needs_timings() says when.
// Results cannot depend on any of this: the rows are the same numbers whichever stream produced them.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace dpr {

class PlacePolicy {
public:
    struct Fixed {                  // decided where the run starts (the environment is read there, once)
        bool allowed = false;       // Mash source, DPR_PLACE_NO_OVERLAP unset, not several ranks on the window transport
        bool always = false;        // allowed and several real ranks
        int64_t multi_min = 150000; // place_multi_min(): first tip of the four-tip launch pairs
        int64_t R = 256;            // rows per batch
    };
    // rows per batch: 1024 for Mash input, whose batches run beside the tree kernels (100 000 unaligned tips: 3.81 / 3.60 /
    // 3.93 s with 256 / 1024 / 4096 -- fewer launch tails, but a longer start-up without overlap); DPR_PLACE_BATCH overrides
    static int64_t batch_rows(bool mash, int64_t env_value) { return env_value >= 16 && env_value <= 65536 ? env_value : mash ? 1024 : 256; }
    static Fixed fixed_for(bool mash, bool several_ranks, bool window_transport, bool no_overlap, int64_t multi_min, int64_t batch_env)
    {
        Fixed f;
        f.allowed = mash && !no_overlap && !(several_ranks && window_transport);
        f.always = f.allowed && several_ranks;
        f.multi_min = multi_min;
        f.R = batch_rows(mash, batch_env);
        return f;
    }
    static double pairs(int64_t i0, int64_t nr) { return (double)nr * ((double)i0 + 0.5 * (double)(nr - 1)); }

    PlacePolicy(const Fixed& f, int64_t last) : f_(f), last_(last) {}
    const Fixed& fixed() const { return f_; }
    bool ahead() const { return ahead_; }                // the batch up next was produced beside its predecessor
    size_t observed() const { return observed_; }        // batches whose timings have been handed in
    // Does decide(i0, nr) read timings?  Then the caller first observes every batch before this one, in order.
    bool needs_timings(int64_t i0, int64_t nr) const { return f_.allowed && i0 + f_.R < last_ && !f_.always && i0 + nr > f_.multi_min; }
    // the next unobserved batch has finished: its tree kernels took tree_ms (negative: unknown), and its rows dist_ms if they were
    // produced alone on the main stream
    void observe(double tree_ms, double dist_ms)
    {
        const Batch& b = batches_[observed_++];
        if (tree_ms >= 0.0 && b.nr > 0) tree_ms_per_tip_ = tree_ms / (double)b.nr / (b.tree_alone ? 1.0 : 1.4);
        if (b.dist_alone && pairs(b.i0, b.nr) >= 5.0e7 && dist_ms > 0.0) pairs_per_ms_ = pairs(b.i0, b.nr) / dist_ms;
    }
    // batch [i0, i0 + nr) is about to be placed: are the rows of its successor [i0 + R, ...) produced beside its tree kernels?
    bool decide(int64_t i0, int64_t nr)
    {
        const int64_t j0 = i0 + f_.R;
        bool next = false;
        if (f_.allowed && j0 < last_) {
            if (f_.always || i0 + nr <= f_.multi_min) next = true;
            else {
                const double est = pairs(j0, last_ - j0 < f_.R ? last_ - j0 : f_.R) / pairs_per_ms_;
                next = tree_ms_per_tip_ > 0.0 ? est < tree_ms_per_tip_ * (double)nr : est < 1.0;
            }
        }
        batches_.push_back({ i0, nr, !ahead_, !next });
        ahead_ = next;
        return next;
    }

private:
    struct Batch { int64_t i0, nr; bool dist_alone, tree_alone; };
    Fixed f_;
    int64_t last_;
    bool ahead_ = false;
    double tree_ms_per_tip_ = -1.0, pairs_per_ms_ = 4.5e6;      // what a batch that ran alone cost
    std::vector<Batch> batches_;
    size_t observed_ = 0;
};

}  // namespace dpr
