"""What the one metadata check of the batch entry points (check_batch in roman_hip.hip) guarantees, at the smallest shape that
exercises it: B = 2, maps of 6 and 5 objects.  Every malformed batch is refused with ROMAN_E_INVALID by every entry point the
condition applies to, before anything is enqueued or a workspace is taken: the same context then completes a valid call whose
result equals the one taken before the refusals.  And the workspace rotation the device-pointer entry points share: calls of
roman_align_batch_dev and roman_mno_batch_dev interleaved at depth 2 equal the same calls at depth 1 bit for bit."""
import numpy as np
import pytest

from _hipmem import Hip
from conftest import registration_for
from roman_amd import _abi, synth
from roman_amd.align import batch as rb
from roman_amd.runtime import Context, RomanHipError, mno_solution_dtype, stats_dtype

pytestmark = pytest.mark.gpu

OK_LIST = np.array([[0, 0], [1, 1], [2, 2], [3, 3]], dtype=np.int32)
OK_ASSOC, OK_OFF = np.concatenate([OK_LIST, OK_LIST]), [0, 4, 8]
RANSAC = _abi.RomanRansacParams(256, 256, 0.95, 0.5, 0.999, 0)


def _n1_negative(a):
    a["n1"][1] = -1


def _off2_negative(a):
    a["off2"][1] = -1


def _past_the_pool(a):
    a["off1"][1] = a["n_objects"] + 1 - a["n1"][1]


def _list_not_from_0(a):
    a["assoc_off"] = [1, 4, 8]


def _list_decreasing(a):
    a["assoc_off"] = [0, 5, 4]


def _index_out_of_range(a):
    a["assoc"], a["assoc_off"] = np.concatenate([OK_LIST, [[6, 0]]]).astype(np.int32), [0, 4, 5]      # i == n1


# the condition, and whether it needs n_objects / an association list / a HOST association list to show
CASES = {"n1[1]=-1": (_n1_negative, ()), "off2[1]=-1": (_off2_negative, ()), "off1[1]+n1[1]=n_objects+1": (_past_the_pool, ("pool",)),
         "assoc_off=[1,4,8]": (_list_not_from_0, ("list",)), "assoc_off=[0,5,4]": (_list_decreasing, ("list",)),
         "association (6,0)": (_index_out_of_range, ("list", "host list"))}
ENTRIES = {"align_batch": ("pool", "list", "host list"), "mno_batch": ("pool", "list", "host list"), "ransac_batch": ("pool",),
           "align_batch_resident": ("list",)}
APPLICABLE = [(e, k) for e in ENTRIES for k in CASES if set(CASES[k][1]) <= set(ENTRIES[e])]


@pytest.fixture(scope="module")
def setup(ctx):
    reg = registration_for("clipper"); reg.set_context(ctx)
    pr = synth.make_pair(6, 5, 0, 36)
    b = rb.batch_from_pairs(reg, [(pr.map1, pr.map2), (pr.map1, pr.map2)])
    hip = Hip()
    dev = dict(feats=hip.upload(b.feats), assoc={})
    P = reg._abi_params()

    def call(entry, **bad):
        a = dict(off1=b.off1.copy(), n1=b.n1.copy(), off2=b.off2.copy(), n2=b.n2.copy(), assoc=OK_ASSOC, assoc_off=OK_OFF, n_objects=b.feats.shape[0])
        if bad:
            bad["change"](a)
        if entry == "align_batch":
            r = ctx.align_batch(P, b.feats, a["off1"], a["n1"], a["off2"], a["n2"], assoc=a["assoc"], assoc_off=a["assoc_off"])
            return [x.tobytes() for x in r.assoc] + [r.T.tobytes(), r.status.tobytes()]
        if entry == "mno_batch":
            r = ctx.mno_batch(P, b.feats, a["off1"], a["n1"], a["off2"], a["n2"], num_solutions=2, assoc=a["assoc"], assoc_off=a["assoc_off"])
            return [x.tobytes() for s in r.assoc for x in s] + [r.score.tobytes(), r.T.tobytes(), r.status.tobytes()]
        if entry == "ransac_batch":
            r = ctx.ransac_batch(RANSAC, b.feats[:, :3], a["off1"], a["n1"], a["off2"], a["n2"])
            return [x.tobytes() for x in r.assoc] + [r.records.tobytes()]
        key = a["assoc"].tobytes()                           # align_batch_resident: the list in device memory (never read by the check)
        if key not in dev["assoc"]:
            dev["assoc"][key] = hip.upload(a["assoc"])
        r = ctx.align_batch_resident(P, dev["feats"], b.feats.shape[1], a["off1"], a["n1"], a["off2"], a["n2"], assoc_ptr=dev["assoc"][key], assoc_off=a["assoc_off"])
        return [x.tobytes() for x in r.assoc] + [r.T.tobytes(), r.status.tobytes()]

    before = {e: call(e) for e in ENTRIES}
    yield call, before
    hip.free_all()


@pytest.mark.parametrize("entry,case", APPLICABLE)
def test_malformed_batch_is_refused_and_the_context_goes_on(setup, entry, case):
    call, before = setup
    with pytest.raises(RomanHipError) as e:
        call(entry, change=CASES[case][0])
    print(e.value)
    assert e.value.code == _abi.ROMAN_E_INVALID
    assert call(entry) == before[entry]


def test_resident_and_host_entry_agree(setup):
    """(the two align entries were given the same valid batch: the refusals above compared each with itself only)"""
    _, before = setup
    assert before["align_batch"] == before["align_batch_resident"]


def _three_calls(depth):
    """align_batch_dev, mno_batch_dev, align_batch_dev without waiting in between, on a context of its own -> the raw outputs."""
    reg = registration_for("clipper")
    pr = synth.make_pair(6, 5, 0, 36)
    b = rb.batch_from_pairs(reg, [(pr.map1, pr.map2), (pr.map1, pr.map2)])
    P, F, B, kmax, K = reg._abi_params(), b.feats.shape[1], 2, b.kmax(), 2
    c, hip = Context(0), Hip()
    try:
        feats = hip.upload(b.feats)
        zeros = lambda nbytes: hip.upload(np.zeros(nbytes, dtype=np.uint8))
        al = [dict(assoc=zeros(B * kmax * 2 * 4), n=zeros(B * 4), T=zeros(B * 16 * 8), status=zeros(B * 4), stats=zeros(B * _abi.STATS_NBYTES)) for _ in range(2)]
        mno = dict(assoc=zeros(B * K * kmax * 2 * 4), sol=zeros(B * K * _abi.MNO_SOLUTION_NBYTES), stats=zeros(B * K * _abi.STATS_NBYTES))
        c.set_pipeline(depth)
        for o in (al[0], None, al[1]):
            if o is None:
                c.mno_batch_dev(P, feats, F, b.off1, b.n1, b.off2, b.n2, K, kmax, mno["assoc"], mno["sol"], mno["stats"])
            else:
                c.align_batch_dev(P, feats, F, b.off1, b.n1, b.off2, b.n2, kmax, o["assoc"], o["n"], o["T"], o["status"], o["stats"])
        c.join()
        c.sync()
        out = []
        for o in al:
            n = hip.download(o["n"], (B,), np.int32); a = hip.download(o["assoc"], (B, kmax, 2), np.int32)
            st = hip.download(o["status"], (B,), np.int32)
            assert not np.any(st & (_abi.ROMAN_ST_WORKSPACE | _abi.ROMAN_ST_INTERNAL))     # (a skipped problem would compare equal too)
            out += [n.tobytes(), st.tobytes(), hip.download(o["T"], (B, 16), np.float64).tobytes(), hip.download(o["stats"], (B,), stats_dtype()).tobytes()]
            out += [a[k, :n[k]].tobytes() for k in range(B)]
        sol = hip.download(mno["sol"], (B, K), mno_solution_dtype())
        assert not np.any(sol["status"] & (_abi.ROMAN_ST_WORKSPACE | _abi.ROMAN_ST_INTERNAL))
        ma = hip.download(mno["assoc"], (B, K, kmax, 2), np.int32)
        out += [sol.tobytes(), hip.download(mno["stats"], (B, K), stats_dtype()).tobytes()]
        out += [ma[k, j, :sol["n_assoc"][k, j]].tobytes() for k in range(B) for j in range(K)]
        c.set_pipeline(1)
        return out
    finally:
        hip.free_all()
        c.close()


def test_align_and_mno_calls_share_the_rotation_at_depth_2():
    assert _three_calls(2) == _three_calls(1)
