"""CPU: the host-side sample tiles of the packed text pass (encoders.text_tiles), the packing ufnd_text_pack_tiles computes."""
import random

import torch

from ultrafnd_git_amd.encoders import TEXT_TILE_ROWS, TEXT_TILE_SAMPLES, text_tile_count, text_tiles


def _plain_ffd(n_rows):
    """first-fit-decreasing without a sample cap: the tile count"""
    free = []
    for n in sorted((int(n) for n in n_rows if n > 0), reverse=True):
        for t, f in enumerate(free):
            if f >= n:
                free[t] -= n
                break
        else:
            free.append(TEXT_TILE_ROWS - n)
    return len(free)


def _check_partition(n_rows, tiles):
    """every live sample once, contiguous rows inside one tile, back to back from row 0, no tile over 256 rows or over the cap"""
    seen = set()
    for tl in tiles:
        assert 1 <= len(tl) <= TEXT_TILE_SAMPLES
        at = 0
        for b, r0 in tl:
            assert b not in seen and n_rows[b] > 0 and r0 == at, (b, r0, at)
            seen.add(b)
            at += n_rows[b]
        assert at <= TEXT_TILE_ROWS
        assert [n_rows[b] for b, _ in tl] == sorted((n_rows[b] for b, _ in tl), reverse=True)
    assert seen == {b for b, n in enumerate(n_rows) if n > 0}
    assert len(tiles) <= (len(n_rows) + 1) // 2      # the capacity the encoder allocates


def test_fixed_mixes():
    assert text_tiles([]) == [] and text_tiles([0, 0]) == []
    assert text_tiles([7]) == [[(0, 0)]]
    assert text_tiles([128] * 5) == [[(0, 0), (1, 128)], [(2, 0), (3, 128)], [(4, 0)]]
    assert text_tiles([10, 128, 0, 70, 40, 128]) == [[(1, 0), (5, 128)], [(3, 0), (4, 70), (0, 110)]]
    assert text_tiles([100, 100, 56]) == [[(0, 0), (1, 100), (2, 200)]]                   # exactly 256 rows
    assert text_tile_count([16] * 16) == 1 and text_tile_count([16] * 17) == 2
    assert text_tile_count([1] * 16) == 1 and text_tile_count([1] * 17) == 2              # the 16-sample cap binds
    assert [len(t) for t in text_tiles([3] * 40)] == [16, 16, 8]


def test_never_more_tiles_than_first_fit_decreasing():
    rng = random.Random(11)
    for _ in range(200):
        n = [rng.randint(16, 128) for _ in range(128)]
        tiles = text_tiles(n)
        assert len(tiles) <= _plain_ffd(n)
        assert len(tiles) >= -(-sum(n) // TEXT_TILE_ROWS)
        _check_partition(n, tiles)


def test_partition_rules_over_every_length():
    rng = random.Random(12)
    for _ in range(300):
        n = [rng.choice([0, rng.randint(1, 128), rng.choice([1, 15, 16, 17, 63, 64, 65, 127, 128])]) for _ in range(rng.randint(1, 60))]
        _check_partition(n, text_tiles(n))


def _bench_group_lengths():
    """the lengths of bench.py's four text groups: make_batches(128, 4, 44) draws, per group and in this order from one seeded generator,
    the ids, the lengths and the other inputs of the batch"""
    g = torch.Generator().manual_seed(44)
    out = []
    for _ in range(4):
        torch.randint(0, 30522, (128, 128), generator=g)
        out.append(torch.randint(16, 129, (128,), generator=g).tolist())
        torch.randn(128, 128, generator=g)
        torch.randn(128, 1, 3, 224, 224, generator=g)
        torch.randn(128, 256, generator=g)
        torch.randn(128, 128, generator=g)
        torch.rand(128, 2, generator=g)
        torch.randint(0, 2, (128,), generator=g)
    return out


def test_the_bench_groups_take_two_rounds():
    groups = _bench_group_lengths()
    assert [sum(n) for n in groups] == [8947, 9941, 9031, 9469]
    for n, most in zip(groups, (36, 40, 36, 38)):
        tiles = text_tiles(n)
        _check_partition(n, tiles)
        assert len(tiles) <= most, (len(tiles), most)
        assert len(tiles) * 12 <= 512
