"""The QUAD shape's compressed corridor copy (solver_ref4.hip: RECT): a batch whose corridors are all rectangles -- four normals
(-S, C), (C, S), (S, -C), (-C, -S) with the same bits of C and S at every point -- is read as 10 doubles per point instead of 16.

Bar: BIT-EQUAL.  Every evaluation and every whole solve on the compressed path equals the same call with DFTPAV_RECT_CORRIDOR=0 (the
sixteen-double layout) and the restatement of the reference (oracle.pyoracle, order 0); a batch that does not qualify falls back to the
sixteen-double layout, says so (dftpav_debug_batch_corridor_layout) and still equals the restatement; the copy and the choice follow
the data from upload to upload.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from dftpav_amd import scenarios as sc

pytestmark = pytest.mark.gpu

KEYS = ("final_cost", "x", "status", "iters", "evals", "hist_sum", "success")


def _layout_of(hiplib, bt):
    fn = hiplib.lib().dftpav_debug_batch_corridor_layout
    fn.argtypes = [C.c_void_p]
    fn.restype = C.c_int
    return int(fn(bt._b))


def _scenario(hiplib, name, B):
    p = hiplib.default_params()
    if name == "cfg3":
        s = sc.baseline_config(3, B=B)                                   # 16 pieces x 33 points, n = 31
    else:
        s = sc.make_scenario([11], [1], 12, 20, B, seed=31, name="n11")   # N < 16, K != Kd: lanes without a piece, rounds without a point
    s.apply_resolution(p)
    return p, s


def _quad_batch(hiplib, monkeypatch, p, s, rect=True):
    """a batch in the reference order, QUAD shape forced (the plan picks it on its own only for large batches)"""
    if rect:
        monkeypatch.delenv("DFTPAV_RECT_CORRIDOR", raising=False)
    else:
        monkeypatch.setenv("DFTPAV_RECT_CORRIDOR", "0")
    h = hiplib.Handle(p)
    bt = hiplib.Batch(h, s.layout, s.B)
    bt.upload(s)
    monkeypatch.delenv("DFTPAV_RECT_CORRIDOR", raising=False)
    monkeypatch.setenv("DFTPAV_REF_SHAPE", "quad")
    bt.set_order(hiplib.ORDER_REFERENCE)
    monkeypatch.delenv("DFTPAV_REF_SHAPE")
    return h, bt


def _points(bt):
    rng = np.random.default_rng(11)
    x0 = bt.x0()
    return [x0, x0 + rng.normal(0, 0.3, x0.shape)]


def _check_against_restatement(oracle, p, s, bt, evals, r, step=1):
    for x, (f, g) in evals:
        for b in range(0, s.B, step):
            fo, go = oracle.OracleProblem(p, s, b, order=0).eval(x[b])
            assert f[b] == fo and np.array_equal(g[b], go), b
    want = oracle.solve_batch(p, s, nthreads=4, order=0)
    for k in KEYS:
        assert np.array_equal(r[k], want[k]), k


@pytest.mark.parametrize("name", ["cfg3", "n11"])
def test_compressed_path_equals_generic_and_restatement(hiplib, oracle, monkeypatch, name):
    p, s = _scenario(hiplib, name, 10)
    h, bt = _quad_batch(hiplib, monkeypatch, p, s)
    hg, bg = _quad_batch(hiplib, monkeypatch, p, s, rect=False)
    xs = _points(bt)
    ev = [(x, bt.eval(x)) for x in xs]
    evg = [(x, bg.eval(x)) for x in xs]
    assert _layout_of(hiplib, bt) == 1, "the compressed copy was not taken"
    assert _layout_of(hiplib, bg) == 0, "the knob did not force the sixteen-double layout"
    for (_, (f, g)), (_, (f2, g2)) in zip(ev, evg):
        assert np.array_equal(f, f2) and np.array_equal(g, g2)
    r, rg = bt.solve(), bg.solve()
    assert _layout_of(hiplib, bt) == 1 and _layout_of(hiplib, bg) == 0
    for k in KEYS:
        assert np.array_equal(r[k], rg[k]), k
    _check_against_restatement(oracle, p, s, bt, ev, r)
    for b_, h_ in ((bt, h), (bg, hg)):
        b_.close()
        h_.close()


def _one_ulp(s):
    """one normal component of one point of one trajectory one ulp off AFTER the upload's normalisation c / sqrt(c0 c0 + c1 c1): the
    raw value is moved until the normalised one (the same IEEE operations, in numpy) differs in its bits"""
    cor = s.corridor.copy()
    b, pt, k = s.B // 2, 17, 2
    c = cor[b, pt, k, :2].copy()
    before = c[0] / np.sqrt(c[0] * c[0] + c[1] * c[1])
    for _ in range(64):
        c[0] = np.nextafter(c[0], np.inf)
        if c[0] / np.sqrt(c[0] * c[0] + c[1] * c[1]) != before:
            break
    else:
        raise AssertionError("the perturbation does not survive the normalisation")
    cor[b, pt, k, 0] = c[0]
    return dataclasses.replace(s, corridor=cor)


def _plus_zero(s):
    """one point's rectangle at yaw 0: S = 0.0, stored as +0.0 in planes 0 and 2 (the relation wants -0.0 in plane 0)"""
    cor = s.corridor.copy()
    cor[1, 5, :, :2] = np.array([[0.0, 1.0], [1.0, 0.0], [0.0, -1.0], [-1.0, 0.0]])
    assert not np.signbit(cor[1, 5, 0, 0]) and not np.signbit(cor[1, 5, 2, 0])
    return dataclasses.replace(s, corridor=cor)


def _planes(H):
    def make(s):
        if H < 4:
            lay = type(s.layout)(s.layout.piece_nums, s.layout.singuls, H=H)
            return dataclasses.replace(s, layout=lay, corridor=np.ascontiguousarray(s.corridor[:, :, :H]))
        cor = np.zeros((s.B, s.n_points, H, 4))
        cor[:, :, :4] = s.corridor
        for k in range(4, H):  # copies of the first planes pulled 0.2 m inwards, so that they are the active ones
            cor[:, :, k] = s.corridor[:, :, k % 4]
            cor[:, :, k, 2:] -= 0.2 * s.corridor[:, :, k % 4, :2]
        lay = type(s.layout)(s.layout.piece_nums, s.layout.singuls, H=H)
        return dataclasses.replace(s, layout=lay, corridor=np.ascontiguousarray(cor))
    return make


@pytest.mark.parametrize("case,change", [("one_ulp", _one_ulp), ("plus_zero", _plus_zero), ("H3", _planes(3)), ("H5", _planes(5))])
def test_batches_that_must_fall_back(hiplib, oracle, monkeypatch, case, change):
    p, s = _scenario(hiplib, "cfg3", 6)
    s = change(s)
    h, bt = _quad_batch(hiplib, monkeypatch, p, s)
    ev = [(x, bt.eval(x)) for x in _points(bt)]
    assert _layout_of(hiplib, bt) == 0, "a batch that is not all rectangles took the compressed copy"
    r = bt.solve()
    assert _layout_of(hiplib, bt) == 0
    _check_against_restatement(oracle, p, s, bt, ev, r)
    bt.close()
    h.close()


def test_nan_normal_keeps_the_generic_layout(hiplib, monkeypatch):
    """a point whose normals are NaNs signed as the four relations want them (a division keeps the sign of a NaN operand where the
    hardware propagates it, so the patterns may well satisfy the relations among themselves) does not take the compressed copy"""
    p, s = _scenario(hiplib, "cfg3", 4)
    cor = s.corridor.copy()
    nan = float("nan")
    cor[2, 9, :, :2] = np.array([[-nan, nan], [nan, nan], [nan, -nan], [-nan, -nan]])
    s = dataclasses.replace(s, corridor=cor)
    h, bt = _quad_batch(hiplib, monkeypatch, p, s)
    bt.eval(bt.x0())
    assert _layout_of(hiplib, bt) == 0
    bt.close()
    h.close()


def test_copy_and_choice_follow_the_data(hiplib, oracle, monkeypatch):
    """rectangles -> a batch with one normal one ulp off -> rectangles again, uploaded into ONE batch"""
    p, s = _scenario(hiplib, "cfg3", 6)
    s_off = _one_ulp(s)
    h, bt = _quad_batch(hiplib, monkeypatch, p, s)
    for want_layout, data in ((1, s), (0, s_off), (1, s), (0, s_off)):
        bt.upload(data)
        assert _layout_of(hiplib, bt) == -1   # the copy is made by the next launch
        x = _points(bt)[1]
        f, g = bt.eval(x)
        assert _layout_of(hiplib, bt) == want_layout
        r = bt.solve()
        assert _layout_of(hiplib, bt) == want_layout
        _check_against_restatement(oracle, p, data, bt, [(x, (f, g))], r, step=2)
    bt.close()
    h.close()
