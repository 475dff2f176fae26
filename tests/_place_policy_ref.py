"""The per-batch overlap policy of k-closest placement (dipper_amd/csrc/place_policy.hpp, table in include/dipper_hip.h) restated
in Python: the reference of the randomised comparison in test_place_policy.py."""


def pairs(i0, nr):
    return nr * (i0 + 0.5 * (nr - 1))


def run(mash, world, window, no_overlap, multi_min, first, last, R, tree_ms, dist_ms):
    allowed = mash and not no_overlap and not (world > 1 and window)
    starts = list(range(first, last, R))
    nrs = [min(R, last - i0) for i0 in starts]
    beside = [False] * len(starts)
    tree_alone = [True] * len(starts)
    for k, (i0, nr) in enumerate(zip(starts, nrs)):
        if not allowed or k + 1 == len(starts):
            continue
        if world > 1 or i0 + nr <= multi_min:
            beside[k + 1] = True
        else:
            per_tip, rate = -1.0, 4.5e6
            for b in range(k):
                per_tip = tree_ms[b] / nrs[b] / (1.0 if tree_alone[b] else 1.4)
                if not beside[b] and pairs(starts[b], nrs[b]) >= 5e7 and dist_ms[b] > 0:
                    rate = pairs(starts[b], nrs[b]) / dist_ms[b]
            est = pairs(starts[k + 1], nrs[k + 1]) / rate
            beside[k + 1] = est < per_tip * nr if per_tip > 0 else est < 1.0
        tree_alone[k] = not beside[k + 1]
    return beside
