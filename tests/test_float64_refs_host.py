"""CPU checks of tests/float64_refs.py, the float64 references tests/test_gpu_optim_resample_float64.py compares the HIP
kernels with: each reference is held against an independent formulation in torch, so that a GPU test cannot pass or fail
because of a mistake in its own yardstick."""
import pytest
import torch
import torch.nn.functional as TF

from tests import float64_refs as R

F64 = torch.float64


def test_chunk_tables_tile_the_arena():
    ct, cb, cl, fc = R.chunk_tables(R.A2_SIZES)
    assert cb[0] == 0 and all(cb[i] + cl[i] == cb[i + 1] for i in range(len(cb) - 1)) and cb[-1] + cl[-1] == sum(R.A2_SIZES)
    assert [fc[t + 1] - fc[t] for t in range(len(R.A2_SIZES))] == [1, 1, 1, 1, 1, 1, 2, 4, 1, 1]
    starts = [sum(R.A2_SIZES[:t]) for t in range(len(R.A2_SIZES))]
    assert {s & 3 for s in starts} == {0, 1, 2, 3}
    for t, s in enumerate(starts):   # no chunk crosses a tensor
        for c in range(fc[t], fc[t + 1]):
            assert ct[c] == t and s <= cb[c] and cb[c] + cl[c] <= s + R.A2_SIZES[t]
    assert sum(R.A2_SIZES) < 1 << 20


@pytest.mark.parametrize("mom,clip,scale", [(0.9, 1.0, 1.0), (0.9, 1.0, 0.125), (0.0, 1.0, 0.5), (0.9, 0.0, 0.5)])
def test_sgd_clip_ref_equals_torch_sgd(mom, clip, scale):
    """sgd_clip_ref against torch.optim.SGD in float64 after per-parameter clip_grad_norm_(p, clip, 2.0) on gradients
    pre-scaled by `scale` (solver/build.py of the reference: one clip call per parameter), three steps, per-tensor weight decay
    through parameter groups; tensors above and below the clip threshold and an all-zero gradient.  1e-12 relative."""
    sizes = R.A2_SIZES
    g = torch.Generator().manual_seed(11)
    lr = 0.1
    wd = [(0.0, 1e-4, 5e-2)[t % 3] for t in range(len(sizes))]
    params = [torch.nn.Parameter(torch.randn(n, generator=g, dtype=F64)) for n in sizes]
    opt = torch.optim.SGD([{"params": [p], "weight_decay": w} for p, w in zip(params, wd)], lr=lr, momentum=mom)
    p = torch.cat([q.detach().clone() for q in params])
    m = torch.zeros_like(p)   # torch's first step: buf = grad, which is mom * 0 + grad
    for it in range(3):
        grads = []
        for t, n in enumerate(sizes):
            gt = torch.randn(n, generator=g, dtype=F64)
            target = (20.0, 0.05)[t % 2] / scale      # ||g|| scale above / below the threshold
            grads.append(gt * 0 if t == 2 else gt * (target / gt.norm()))
        for q, gt in zip(params, grads):
            q.grad = gt * scale
            if clip > 0:
                torch.nn.utils.clip_grad_norm_(q, clip, 2.0)
        opt.step()
        p, m = R.sgd_clip_ref(p, torch.cat(grads), m, sizes, wd, lr, mom, clip, scale)
        want_p = torch.cat([q.detach() for q in params])
        assert float((p - want_p).abs().max()) <= 1e-12 * float(want_p.abs().max()), it
        if mom:
            want_m = torch.cat([opt.state[q]["momentum_buffer"] for q in params])
            assert float((m - want_m).abs().max()) <= 1e-12 * float(want_m.abs().max()), it


@pytest.mark.parametrize("shape", [(2, 64, 13, 18), (1, 8, 1, 1), (1, 8, 2, 1), (3, 16, 1, 7), (2, 32, 14, 2), (1, 24, 5, 5)])
def test_slots_from_indices_equals_brute_force(shape):
    """The conversion of max_pool2d's return_indices to window slots against a scan of the nine taps (first maximum wins),
    on the tie-quantised input: every window holds ties, many hold negative values only."""
    x = R.tie_values(shape, torch.Generator().manual_seed(sum(shape)), "cpu")
    y, ind = TF.max_pool2d(x, 3, 2, 1, return_indices=True)
    best, slot = R.brute_force_slots(x)
    assert torch.equal(y, best)
    assert torch.equal(R.slots_from_indices(ind, shape[3]), slot)
    # the band form (explicit -inf rows, no vertical padding) names the same slots
    xb = TF.pad(x, (0, 0, 1, 1), value=float("-inf"))
    if xb.shape[2] >= 3:
        yb, indb = TF.max_pool2d(xb, 3, 2, (0, 1), return_indices=True)
        n = yb.shape[2]
        assert torch.equal(yb, best[:, :, :n]) and torch.equal(R.slots_from_indices(indb, shape[3], row_off=0), slot[:, :, :n])


def test_stem_unfold_ref_reproduces_conv2d():
    """unfold + the (kh, kw, c) reordering, multiplied by weight.permute(0, 2, 3, 1).reshape(64, 147), is conv2d(7x7, stride 2,
    pad 3) in float64; pixels outside the images and the conv padding give exact zeros."""
    g = torch.Generator().manual_seed(5)
    imgs = [torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8) for h, w in ((50, 70), (64, 61), (1, 1), (16, 32))]
    mean, std = torch.tensor([123.675, 116.28, 103.53]), torch.tensor([58.395, 57.12, 57.375])
    canvas, inside = R.stem_canvas(imgs, mean, std, 64, 96)
    w = torch.randn((64, 3, 7, 7), generator=g, dtype=F64)
    cols = R.stem_unfold_ref(canvas)
    assert cols.shape == (4, 32 * 48, 147)
    got = (cols @ w.permute(0, 2, 3, 1).reshape(64, 147).t()).view(4, 32, 48, 64).permute(0, 3, 1, 2)
    want = TF.conv2d(canvas, w, None, 2, 3)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool((cols[R.stem_unfold_ref(inside) == 0] == 0).all())
    # image 2 is one pixel: only the windows that contain canvas pixel (0, 0) see it, at tap (3 - 2 oy, 3 - 2 ox)
    one = cols[2].view(32, 48, 7, 7, 3)
    assert int((one != 0).any(-1).sum()) == 4 and bool((one[1, 1, 1, 1] == canvas[2, :, 0, 0]).all())
