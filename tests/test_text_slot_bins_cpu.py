"""CPU: the host-side slot bin list of the packed text pass (encoders.text_slot_bins), the layout ufnd_text_pack_bins writes."""
import random

from ultrafnd_git_amd.encoders import text_slot_bin_count, text_slot_bins


def _slots(n):
    return (n + 31) // 32


def test_bin_counts_of_fixed_mixes():
    assert text_slot_bin_count([]) == 0
    assert text_slot_bin_count([0, 0]) == 0
    assert text_slot_bin_count([1]) == 1
    assert text_slot_bin_count([128] * 5) == 5
    assert text_slot_bin_count([32] * 9) == 3          # 1-slot samples four to a bin
    assert text_slot_bin_count([33] * 5) == 3          # 2 + 2, 2 + 2, 2
    assert text_slot_bin_count([65, 65, 1]) == 2       # 3 + 1, 3 alone
    assert text_slot_bin_count([40, 1, 1, 1]) == 2     # 2 + 1 + 1, 1
    assert text_slot_bin_count([31, 32, 33, 63, 64, 65, 95, 96, 97, 128]) == 7
    assert text_slot_bins([10, 128, 70, 40]) == [[(1, 0), (1, 1), (1, 2), (1, 3)], [(2, 0), (2, 1), (2, 2), (0, 0)], [(3, 0), (3, 1), None, None]]


def test_bins_are_an_optimal_partition_with_full_bins_first():
    rng = random.Random(5)
    for _ in range(3000):
        n = [rng.choice([0, rng.randint(1, 128), rng.choice([1, 31, 32, 33, 64, 65, 96, 97, 128])]) for _ in range(rng.randint(1, 50))]
        bins = text_slot_bins(n)
        assert len(bins) == text_slot_bin_count(n)
        total = sum(_slots(x) for x in n)
        # optimal: the 3-slot samples without a 1-slot partner need a bin each, otherwise the slot total sets the count
        n1, n3 = sum(_slots(x) == 1 for x in n), sum(_slots(x) == 3 for x in n)
        assert len(bins) == max(-(-total // 4), sum(_slots(x) == 4 for x in n) + n3 + (-(-(sum(_slots(x) == 2 for x in n) * 2 - 0 + max(n1 - n3, 0)) // 4)))
        seen = {}
        partial = False
        for i, bn in enumerate(bins):
            used = [x is not None for x in bn]
            assert len(bn) == 4 and used[0] and used == sorted(used, reverse=True)
            assert not (partial and all(used))
            partial = partial or not all(used)
            for j, x in enumerate(bn):
                if x is not None:
                    seen.setdefault(x[0], []).append((i, j, x[1]))
        for b, x in enumerate(n):
            if _slots(x) == 0:
                assert b not in seen
                continue
            sl = seen[b]
            assert len({i for i, _, _ in sl}) == 1 and [s for _, _, s in sl] == list(range(_slots(x)))
            assert [j for _, j, _ in sl] == list(range(sl[0][1], sl[0][1] + _slots(x)))
