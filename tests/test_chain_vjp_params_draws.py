"""CPU check of the draws of tests/test_gpu_chain_vjp_params.py: for every case of its closed-form tests, reference (a) with every
stage input taken from the FLOAT32 oracle holds the Float32 bar (1e-3 of max(|cotangent|, max |summand|)) against the Float64 one —
so the reference itself is tame at those draws and a GPU failure there is the kernel's.  Also: in the central-difference cases
every LeakyReLU input stays at least ten steps away from the kink."""
import numpy as np
import pytest

pytest.importorskip("torch")

import test_gpu_chain_vjp_params as t  # noqa: E402


def _cases():
    for law in sorted(t.LAWS):
        for src in "sr":
            for lbar in (True, False):
                for dim, N in ((64, 257), (5, 63)):
                    yield law, src, dim, N, lbar
    for law, src in (("leaky_affine", "r"), ("logit_scale_inv", "r"), ("affine", "r"), ("scale", "s")):
        for dim in (1, 3, 4, 5, 64, 67, 260):
            for N in (1, 63, 65, 1000):
                yield law, src, dim, N, True


def test_float32_oracle_holds_the_bar_on_the_draws():
    from oracle import oracle as orc

    worst = 0.0
    for law, src, dim, N, lbar in _cases():
        stages, X, G, lb = t.draw_case(law, src, dim, N, np.float32, lbar)
        _, r64 = t.ref_closed(orc, stages, X, G, lb)
        _, r32 = t.ref_closed(orc, stages, X, G, lb, fwd_dtype=np.float32)
        for i in r64:
            a, ts = r64[i]
            scale = max(float(np.abs(np.asarray(a)).max()), ts)
            if scale == 0.0:
                continue
            e = float(np.abs(np.asarray(a) - np.asarray(r32[i][0])).max()) / scale
            worst = max(worst, e)
            assert e <= 1e-3, (law, src, dim, N, lbar, i, e)
    print("worst Float32-oracle error on the term scale:", worst)


def test_central_difference_draws_stay_off_the_leaky_relu_kink():
    from oracle import oracle as orc

    for law in ("leaky", "affine_leaky_affine4"):
        for src in "rs":
            stages, X, G, lb = t.draw_case(law, src, 5, 33, np.float64, True, tag="fd")
            u = X
            for op, p0, p1 in stages:
                if op == "leaky":
                    assert np.abs(u).min() >= 1e-5, (law, src, float(np.abs(u).min()))
                u = np.asarray(orc.chain([(t.KIND[op], p0, p1)], np.asfortranarray(u), fused=True)[0], np.float64)
