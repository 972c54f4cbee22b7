"""GPU: the fused recurrent acting step, straight through the C ABI, at every launch shape of its host dispatch.  Each case of
tests/rec_step_model.py runs through the exact-f32 entry (mava_rec_step_f32 / mava_rec_step_continuous_f32) and through
mava_rec_step_packed_f32 on weights packed by mava_rec_step_pack_f32; mava_debug_rec_step_last_instance() must report the
instance the model predicts - rec_step_kernel<NOA> or rec_step_h2_kernel<NOA, RT> - so that the f16x2 kernel cannot be mistaken
for its silent f32 fallback.  New hidden states, values, log-probabilities and continuous actions are held to the float64
reference at 1e-5 (conftest.assert_close) in both kernels; sampled actions are exact on decided rows (rec_step_model.case),
greedy ones everywhere.  Every output buffer holds a sentinel before the launch and is followed by a sentinel-filled guard tile;
every input is compared with its copy afterwards; a second launch must give the same bits.
Measured on an MI355X (largest over all cases, assert_close's form; DESIGN.md section 4 has them per family): hidden states
2.95e-06 (exact f32) and 3.51e-06 (f16x2), values 1.37e-06 and 1.82e-06, log-probabilities 4.45e-07 and 5.99e-07."""
import numpy as np
import pytest
import torch

from oracle import tanh_normal as tn
from tests import rec_step_model as m
from tests import seq_model as sm
from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

SENT = 12345.0
H = m.H
NAMES = sorted(m.CASES)


def _L():
    from mava_amd._lib import check, lib, ptr, stream_ptr

    return lib(), check, ptr, stream_ptr()


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _out(n, width, dev, dtype=torch.float32):
    """n output elements holding the sentinel and one guard tile (32 x width) behind them."""
    return torch.full((int(n) + 32 * int(width),), SENT, device=dev).to(dtype)


def _take(t, n, what):
    a = t.cpu().numpy()
    sent = np.asarray(SENT).astype(a.dtype)
    assert (a[n:] == sent).all(), f"{what}: wrote past its {n} elements"
    assert not (a[:n] == sent).any(), f"{what}: {int((a[:n] == sent).sum())} of {n} elements were never written"
    return a[:n]


def _same_bits(got, want, what):
    for k in want:
        if k != "inst":
            a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
            assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
            bad = a.view(np.uint32) != b.view(np.uint32)
            assert not bad.any(), f"{what}: {k} differs in {int(bad.sum())} of {bad.size} elements, first at {np.argwhere(bad)[0].tolist()}"


def _inputs(dev, c):
    """Device copies of a case's inputs, the two weight packs (each followed by guard bytes) and a second copy of everything."""
    L, check, ptr, s = _L()
    sp = c["spec"]
    d = dict(pa=_d(c["pa"], dev), pc=_d(c["pc"], dev), x=_d(c["x"], dev), xc=_d(c["xc"], dev), ha=_d(sm.to_t32(c["ha"]), dev),
             hc=_d(sm.to_t32(c["hc"]), dev), done_a=_d(c["done_a"], dev))
    d["done_c"] = d["done_a"] if sp.form == "env" else _d(c["done_c"], dev)
    d["mask"] = None if c["mask"] is None else _d(c["mask"].astype(np.uint8), dev)
    for k, params, din in (("pack_a", d["pa"], sp.din_a), ("pack_c", d["pc"], sp.din_c)):
        nbytes = L.mava_rec_step_pack_bytes(din)
        assert nbytes == (4 * ((din + 15) // 16) + 224) * 2048
        d[k] = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=dev)
        check(L.mava_rec_step_pack_f32(ptr(params), din, ptr(d[k]), s), "mava_rec_step_pack_f32")
        torch.cuda.synchronize()
        assert (d[k][nbytes:] == 0xA5).all(), "the pack kernel wrote past mava_rec_step_pack_bytes"
    d["copy"] = {k: v.clone() for k, v in d.items() if v is not None}
    return d


def _launch(dev, c, d, entry, greedy):
    """One launch; returns the reported instance and the outputs (guard tiles and sentinels checked)."""
    L, check, ptr, s = _L()
    sp = c["spec"]
    Ra, Rc, n, vb = c["rows_a"], c["rows_c"], sp.n, c["vbroadcast"]
    ha, hc = _out(Ra * H, H, dev), _out(Rc * H, H, dev)
    logp, value = _out(Ra, 1, dev), _out(Rc * vb, vb, dev)
    act = _out(Ra * n, n, dev) if sp.cont else _out(Ra, 1, dev, torch.int32)
    rng_args = (m.SEED, m.STEP, sp.row_offset, greedy)
    critic = (ptr(d["pc"]), sp.din_c, ptr(d["xc"]), c["share"], ptr(d["done_c"]), c["done_stride"], ptr(d["hc"]), ptr(hc), Rc, vb,
              ptr(value), s)
    if entry == "packed":
        check(L.mava_rec_step_packed_f32(ptr(d["pack_a"]), ptr(d["pack_c"]), ptr(d["pa"]), sp.din_a, n, tn.MIN_SCALE, ptr(d["x"]),
                                         ptr(d["mask"]), ptr(d["done_a"]), ptr(d["ha"]), ptr(ha), Ra, *rng_args,
                                         None if sp.cont else ptr(act), ptr(act) if sp.cont else None, ptr(logp), *critic),
              "mava_rec_step_packed_f32")
    elif sp.cont:
        check(L.mava_rec_step_continuous_f32(ptr(d["pa"]), sp.din_a, n, tn.MIN_SCALE, ptr(d["x"]), ptr(d["done_a"]), ptr(d["ha"]), ptr(ha),
                                             Ra, *rng_args, ptr(act), ptr(logp), *critic), "mava_rec_step_continuous_f32")
    else:
        check(L.mava_rec_step_f32(ptr(d["pa"]), sp.din_a, n, ptr(d["x"]), ptr(d["mask"]), ptr(d["done_a"]), ptr(d["ha"]), ptr(ha), Ra,
                                  *rng_args, ptr(act), ptr(logp), *critic), "mava_rec_step_f32")
    inst = L.mava_debug_rec_step_last_instance()
    torch.cuda.synchronize()
    o = dict(inst=inst, ha=_take(ha, Ra * H, "actor hidden state"), hc=_take(hc, Rc * H, "critic hidden state"),
             logp=_take(logp, Ra, "log_prob"), value=_take(value, Rc * vb, "value"),
             action=_take(act, Ra * n if sp.cont else Ra, "action"))
    return o


_PRIMER = {}


def _prime(dev):
    """A one-tile launch of rec_step_h2_kernel<8, 1>: the export then holds 2081, an id that no exact-f32 launch reports - the
    next launch is seen to set it, not to have left it."""
    L, check, ptr, s = _L()
    if not _PRIMER:
        rng = np.random.default_rng(1)
        p = _d(m._params(rng, 1, 2), dev)
        q = _d(m._params(rng, 1, 1), dev)
        pk = [torch.zeros(L.mava_rec_step_pack_bytes(1), dtype=torch.uint8, device=dev) for _ in range(2)]
        check(L.mava_rec_step_pack_f32(ptr(p), 1, ptr(pk[0]), s), "pack")
        check(L.mava_rec_step_pack_f32(ptr(q), 1, ptr(pk[1]), s), "pack")
        z = lambda k, dt=torch.float32: torch.zeros(k, dtype=dt, device=dev)
        _PRIMER.update(p=p, q=q, pk=pk, x=z(32), done=z(32, torch.uint8), h=z(32 * H), h2=z(32 * H), h3=z(32 * H), a=z(32, torch.int32), lp=z(32), v=z(32))
    P = _PRIMER
    check(L.mava_rec_step_packed_f32(ptr(P["pk"][0]), ptr(P["pk"][1]), ptr(P["p"]), 1, 2, 0.0, ptr(P["x"]), None, ptr(P["done"]), ptr(P["h"]),
                                     ptr(P["h2"]), 32, 1, 0, 0, 0, ptr(P["a"]), None, ptr(P["lp"]), ptr(P["q"]), 1, ptr(P["x"]), 1, ptr(P["done"]),
                                     1, ptr(P["h"]), ptr(P["h3"]), 32, 1, ptr(P["v"]), s), "primer")
    assert L.mava_debug_rec_step_last_instance() == m.step_id(m.H2, 8, 1)


def _compare(c, o, greedy, what):
    """Prints the case's largest errors (assert_close's form), then asserts."""
    sp = c["spec"]
    Ra, Rc, n, vb = c["rows_a"], c["rows_c"], sp.n, c["vbroadcast"]
    ha, hc = sm.from_t32(o["ha"], Ra, H), sm.from_t32(o["hc"], Rc, H)
    value = o["value"].reshape(Rc, vb)
    r = np.arange(Ra)
    if sp.cont:
        a = o["action"].reshape(Ra, n)
        lp_want = tn.log_prob_terms(sm.f64(a), c["y"], c["scale"])[0].sum(-1)  # of the kernel's own action
    else:
        a = o["action"]
        assert ((a >= 0) & (a < n)).all(), f"{what}: an action outside [0, {n})"
        lp_want = c["logp"][r, a]  # of the kernel's own action
    errs = dict(ha=sm.rel_err(ha, c["ha_new"]), hc=sm.rel_err(hc, c["hc_new"]), value=sm.rel_err(value[:, 0], c["value"]))
    if n > 1 or sp.cont:
        errs["logp"] = sm.rel_err(o["logp"], lp_want)
    if sp.cont:
        errs["action"] = sm.rel_err(a, c["action"][greedy])
    print(f"REC_STEP_ERR {sp.family} {what} " + " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    assert_close(ha, c["ha_new"], m.RTOL, f"{what}: actor hidden state")
    assert_close(hc, c["hc_new"], m.RTOL, f"{what}: critic hidden state")
    assert_close(value[:, 0], c["value"], m.RTOL, f"{what}: value")
    assert (value.view(np.uint32) == value[:, :1].view(np.uint32)).all(), f"{what}: the broadcast copies of a value differ"
    assert_close(o["logp"], lp_want, m.RTOL, f"{what}: log_prob of the kernel's own action")
    if sp.cont:
        assert_close(a, c["action"][greedy], m.RTOL, f"{what}: action = tanh(mean + scale eps)")
        return
    dead = c["dead"]
    if c["mask"] is not None:
        assert c["mask"][r, a][~dead].all(), f"{what}: an illegal action"
    if dead.any():  # a row without a legal action: action 0 and -log(n)
        assert (a[dead] == 0).all() and (np.abs(o["logp"][dead] + np.log(n)) <= 1e-5).all(), what
    if greedy:
        assert np.array_equal(a, c["greedy"]), f"{what}: {int((a != c['greedy']).sum())} greedy actions differ"
    else:
        dec = c["decided"]
        assert np.array_equal(a[dec], c["sampled"][dec]), f"{what}: {int((a[dec] != c['sampled'][dec]).sum())} sampled actions of decided rows differ"


@pytest.mark.parametrize("name", NAMES)
def test_rec_step(dev, name):
    c = m.case(name)
    sp = c["spec"]
    d = _inputs(dev, c)
    outs = {}
    for greedy in sp.greedy:
        for entry in ("f32", "packed"):
            _prime(dev)
            what = f"{name} {entry} greedy={greedy}"
            o = _launch(dev, c, d, entry, greedy)
            want = m.predicted(name, entry == "packed")
            assert o["inst"] == want, f"{what}: instance {o['inst']} ran, {want} expected"
            assert (o["inst"] // 1000 == m.H2) == (entry == "packed" and sp.expect_h2)
            _compare(c, o, greedy, what)
            _same_bits(_launch(dev, c, d, entry, greedy), o, f"{what}: second launch")
            outs[entry, greedy] = o
        if not sp.expect_h2:  # the silent fallback IS the exact-f32 kernel
            _same_bits(outs["packed", greedy], outs["f32", greedy], f"{name} greedy={greedy}: packed entry against mava_rec_step_f32")
    for k, v in d["copy"].items():
        assert torch.equal(d[k], v), f"{name}: input {k} was modified"
