"""-m gpu: ``ta_attention_extend`` (csrc/attention_extend.hip) against ``tests/attention_ref.attend`` in float64.

The reference sees one sequence per row: the Lp prompt slots of the row's clip followed by the row's own T slots; the test builds the
visibility matrix itself (prompt mask for every query, then causal over the row's own valid slots; nothing for queries behind the row's
end) and never asks the library what is visible.  Gate: ``attention_ref.gate`` at the project's factor 2 over the reference's own
rounding model (P~ -> bf16 before P V, the denominator summing the rounded values, O -> bf16), on the rows that have a visible key;
LSE: absolute error within twice the model's plus 2e-5 (f32 accumulation of a 128-term score, which the float64 model does not have).
Exact checks, bit for bit: masked slots refilled with other finite garbage change nothing; the cache shared through ``clip_of`` equals the
cache physically repeated per row; query rows behind a row's end are exact zeros.  Outputs are pre-filled with 7.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attention_ref as R

DEV, BF16, HD = "cuda", torch.bfloat16, 128
SCALE = HD ** -0.5
B = 3
ROWS_OF_CLIP = (3, 0, 1)                 # clip 1 has no candidate
LPS = (1, 31, 32, 33, 150, 200)
HEADS = {1: (2, 2), 2: (4, 2), 4: (4, 1)}


def _lens(T):
    return [T, 1, max(1, T // 2 + 1), max(1, T - 1)]          # ragged; includes 1 and T


def _case(grp, T, Lp, seed, zero_clip=None):
    Hq, Hkv = HEADS[grp]
    clip_of = [b for b, n in enumerate(ROWS_OF_CLIP) for _ in range(n)]
    Rr, Lmax = len(clip_of), Lp + 5                         # Lmax > Lp: the cache has slots the prompt pass never filled
    g = torch.Generator(device="cpu").manual_seed(4000 + seed)
    rnd = lambda *s, sc=1.0: (sc * torch.randn(*s, generator=g)).to(BF16)  # noqa: E731
    Q, Kn, Vn = rnd(Rr, Hq, T, HD, sc=R.QK_SCALE), rnd(Rr, Hkv, T, HD, sc=R.QK_SCALE), rnd(Rr, Hkv, T, HD)
    Kc, Vc = rnd(B, Hkv, Lmax, HD, sc=R.QK_SCALE), rnd(B, Hkv, Lmax, HD)
    pmask = torch.ones(B, Lp, dtype=torch.int32)
    pmask[0, :min(37, Lp - 1)] = 0                          # left padding 37 (as much of it as leaves one prompt token) on clip 0, none on clip 2
    if zero_clip is not None:
        pmask[zero_clip] = 0                                # no prompt slot of this clip is visible at all
    return dict(Hq=Hq, Hkv=Hkv, T=T, Lp=Lp, Lmax=Lmax, R=Rr, Q=Q, Kn=Kn, Vn=Vn, Kc=Kc, Vc=Vc, pmask=pmask,
                clip_of=torch.tensor(clip_of, dtype=torch.int32), lens=torch.tensor(_lens(T), dtype=torch.int32))


def _reference(c):
    """-> (exact O, model O, exact LSE, model LSE, live [R, T]) with O [R*T, Hq*HD], LSE [R, Hq, T]."""
    Rr, T, Lp, Hq, Hkv = c["R"], c["T"], c["Lp"], c["Hq"], c["Hkv"]
    clip, lens = c["clip_of"].long(), c["lens"].long()
    Lt = Lp + T
    q = torch.cat([torch.zeros(Rr, Hq, Lp, HD, dtype=R.F64), c["Q"].to(R.F64)], 2)
    k = torch.cat([c["Kc"][clip][:, :, :Lp].to(R.F64), c["Kn"].to(R.F64)], 2)
    v = torch.cat([c["Vc"][clip][:, :, :Lp].to(R.F64), c["Vn"].to(R.F64)], 2)
    vis = torch.zeros(Rr, Lt, Lt, dtype=torch.bool)
    t = torch.arange(T)
    for r in range(Rr):
        live = t < lens[r]
        vis[r, Lp:, :Lp] = live[:, None] & (c["pmask"][clip[r]] != 0)[None, :]
        vis[r, Lp:, Lp:] = live[:, None] & (t[None, :] <= t[:, None]) & (t[None, :] < lens[r])
    cut = lambda o: o.reshape(Rr, Lt, -1)[:, Lp:].reshape(Rr * T, -1)  # noqa: E731
    (oe, le), (om, lm) = R.attend(q, k, v, vis), R.attend(q, k, v, vis, rounded=True)
    return cut(oe), cut(om), le[:, :, Lp:], lm[:, :, Lp:], (t[None, :] < lens[:, None])


def _run(c, **over):
    from tiny_audio_amd import ops
    a = dict(c, **over)
    d = lambda x: x.to(DEV).contiguous()  # noqa: E731
    out = torch.full((a["Q"].shape[0] * c["T"], c["Hq"] * HD), 7.0, dtype=BF16, device=DEV)
    O, lse = ops.attention_extend(d(a["Q"]), d(a["Kn"]), d(a["Vn"]), d(a["Kc"]), d(a["Vc"]), d(a["pmask"]), d(a["clip_of"]), d(a["lens"]), SCALE,
                                  out=out)
    torch.cuda.synchronize()
    return O.cpu(), lse.cpu()


def _garbage(like, sign):
    """Finite garbage of magnitude 1e4 with alternating sign."""
    alt = torch.ones(like.numel())
    alt[1::2] = -1
    return (sign * 1.0e4 * alt).reshape(like.shape).to(BF16)


@pytest.mark.parametrize("T", (1, 2, 15, 16, 17, 33, 64, 256))
@pytest.mark.parametrize("grp", (1, 2, 4))
def test_extend_against_the_float64_reference(grp, T):
    for i, Lp in enumerate(LPS):
        c = _case(grp, T, Lp, seed=100 * grp + 10 * i + T)
        O, lse = _run(c)
        oe, om, le, lm, live = _reference(c)
        rows = live.reshape(-1)
        assert torch.isfinite(O.float()).all()
        assert not O[~rows].float().any(), "query rows behind the row's end must be exactly 0"
        assert (lse[~live[:, None, :].expand_as(lse)] == 1.0e30).all()
        ok, ratio, worst = R.gate(O[rows], oe[rows], om[rows])
        print(f"EXTEND g{grp}-T{T}-Lp{Lp} O e/m={ratio:.3f}")
        assert ok, (grp, T, Lp, ratio, worst)
        has = live[:, None, :].expand_as(lse)
        bound, err = float((lm[has] - le[has]).abs().max()), float((lse.double()[has] - le[has]).abs().max())
        assert err <= 2 * bound + 2e-5, (grp, T, Lp, "LSE", err, bound)

        # masked prompt slots (pmask == 0, slots >= Lp) and candidate slots >= len refilled with other garbage: the same bits
        clip, lens = c["clip_of"].long(), c["lens"].long()
        dead_p = torch.ones(B, c["Lmax"], dtype=torch.bool)
        dead_p[:, :Lp] = c["pmask"] == 0
        dead_c = torch.arange(T)[None, :] >= lens[:, None]
        Kc2, Vc2, Kn2, Vn2 = c["Kc"].clone(), c["Vc"].clone(), c["Kn"].clone(), c["Vn"].clone()
        mp, mc = dead_p[:, None, :, None].expand_as(Kc2), dead_c[:, None, :, None].expand_as(Kn2)
        Kc2[mp], Vc2[mp] = _garbage(Kc2, 1)[mp], _garbage(Vc2, -1)[mp]
        Kn2[mc], Vn2[mc] = _garbage(Kn2, -1)[mc], _garbage(Vn2, 1)[mc]
        O2, lse2 = _run(c, Kc=Kc2, Vc=Vc2, Kn=Kn2, Vn=Vn2)
        assert torch.equal(O2, O) and torch.equal(lse2, lse), (grp, T, Lp, "garbage in masked slots changed the result")

        # the cache physically repeated per row, clip_of = arange: the same bits as the shared read
        O3, lse3 = _run(c, Kc=c["Kc"][clip], Vc=c["Vc"][clip], pmask=c["pmask"][clip], clip_of=torch.arange(c["R"], dtype=torch.int32))
        assert torch.equal(O3, O) and torch.equal(lse3, lse), (grp, T, Lp, "shared and repeated prompt caches differ")


def test_rows_of_a_clip_without_visible_prompt_see_only_themselves():
    """Clip 2's pmask row is all zero: its candidate's first token sees exactly one key (itself), so O[t = 0] is V[0] bit for bit."""
    c = _case(2, 17, 33, seed=7, zero_clip=2)
    O, _ = _run(c)
    oe, om, _, _, live = _reference(c)
    rows = live.reshape(-1)
    assert R.gate(O[rows], oe[rows], om[rows])[0] and not O[~rows].float().any()
    r = 3                                                   # the row of clip 2
    got = O.reshape(c["R"], c["T"], c["Hq"], HD)[r, 0]
    want = c["Vn"][r, :, 0].repeat_interleave(c["Hq"] // c["Hkv"], 0)
    assert torch.equal(got, want)
