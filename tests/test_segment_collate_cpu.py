"""Host half of rad_mmm_amd.data.SegmentCollate without a GPU: plan_segments (starts, counts, lens, refusals),
segment_layout and stage_segments (only the cropped ranges are staged, and they equal the numpy slices)."""
import numpy as np
import pytest
import torch

from rad_mmm_amd.data import plan_segments, segment_layout, stage_segments

HOP, NFFT, SEG = 256, 1024, 1024
SIZES = (2048, 700, 5000)


def _items(dtype, sizes=SIZES, seed=0):
    g = np.random.default_rng(seed)
    if dtype == np.int16:
        return [{"audio": g.integers(-32768, 32768, s, dtype=np.int16)} for s in sizes]
    return [{"audio": g.uniform(-1, 1, s).astype(np.float32)} for s in sizes]


def test_fixed_starts_counts_lens_and_offsets():
    items = _items(np.int16)
    plan = plan_segments(items, HOP, NFFT, SEG, starts=[100, 0, 4200])
    assert plan.starts.tolist() == [100, 0, 4200]
    assert plan.counts.tolist() == [1024, 700, 800]            # a full segment, the short item whole, a cut tail
    assert plan.lens.tolist() == [4, 2, 3]                     # min(S - start, segment) // hop
    assert plan.offsets.tolist() == [0, 1024, 1024 + 704]      # 16-byte aligned item starts
    assert plan.n_samples == 1024 + 704 + 800 and plan.audio_dtype == np.int16 and plan.segment_size == SEG


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_staged_samples_are_the_numpy_slices_and_nothing_else(dtype):
    items = _items(dtype)
    starts = [100, 0, 4200]
    plan = plan_segments(items, HOP, NFFT, SEG, starts=starts)
    off, total = segment_layout(plan)
    item = np.dtype(dtype).itemsize
    assert off["audio"][1] == plan.n_samples * item
    assert total == 32 + 32 + plan.n_samples * item            # offsets, the two count rows (padded to 16 bytes), the crops
    assert total < sum(SIZES) * item / 2                       # the whole items were never staged
    hb = np.full(total + 64, 0xAB, dtype=np.uint8)
    assert stage_segments(plan, items, hb) == total
    assert (hb[total:] == 0xAB).all()
    o, n = off["audio"]
    audio = hb[o:o + n].view(dtype)
    for b, it in enumerate(items):
        s, c, at = starts[b], int(plan.counts[b]), int(plan.offsets[b])
        assert np.array_equal(audio[at:at + c], it["audio"][s:s + c]), b
    o, n = off["offsets"]
    assert hb[o:o + n].view(np.int64).tolist() == plan.offsets.tolist()
    o, n = off["lens"]
    assert hb[o:o + n].view(np.int32).reshape(2, 3).tolist() == [plan.counts.tolist(), plan.lens.tolist()]


def test_drawn_starts_are_uniform_over_the_allowed_range_and_reproducible():
    items = _items(np.float32, sizes=(1027, 700, 5000))
    g = torch.Generator().manual_seed(4)
    seen = [plan_segments(items, HOP, NFFT, SEG, generator=g).starts for _ in range(200)]
    s = np.stack(seen)
    assert set(s[:, 0]) == {0, 1, 2, 3}                        # 0 .. S - segment, both ends included
    assert (s[:, 1] == 0).all()                                # shorter than the segment: staged whole
    assert s[:, 2].min() >= 0 and s[:, 2].max() <= 5000 - SEG and len(set(s[:, 2])) > 100
    again = plan_segments(items, HOP, NFFT, SEG, generator=torch.Generator().manual_seed(4)).starts
    assert again.tolist() == seen[0].tolist()
    full = plan_segments(items, HOP, NFFT, SEG, generator=g)
    assert full.counts.tolist() == [SEG, 700, SEG] and full.lens.tolist() == [4, 2, 4]


def test_refusals():
    with pytest.raises(ValueError, match="512"):
        plan_segments(_items(np.int16, sizes=(2048, 512)), HOP, NFFT, SEG)
    plan_segments(_items(np.int16, sizes=(2048, 513)), HOP, NFFT, SEG)
    mixed = _items(np.int16, sizes=(2048,)) + _items(np.float32, sizes=(2048,))
    with pytest.raises(ValueError, match="mixed"):
        plan_segments(mixed, HOP, NFFT, SEG)
    with pytest.raises(ValueError, match="starts"):
        plan_segments(_items(np.int16), HOP, NFFT, SEG, starts=[0, 0])
    with pytest.raises(ValueError, match="outside"):
        plan_segments(_items(np.int16), HOP, NFFT, SEG, starts=[0, 700, 0])
    with pytest.raises(ValueError, match="leaves 500 samples"):
        plan_segments(_items(np.int16), HOP, NFFT, SEG, starts=[0, 0, 4500])
    with pytest.raises(ValueError, match="multiple of hop_length"):
        plan_segments(_items(np.int16), HOP, NFFT, 1000)
    with pytest.raises(ValueError, match="int16 or float32"):
        plan_segments([{"audio": np.zeros(2048, dtype=np.float64)}], HOP, NFFT, SEG)
    with pytest.raises(ValueError, match="empty"):
        plan_segments([], HOP, NFFT, SEG)
