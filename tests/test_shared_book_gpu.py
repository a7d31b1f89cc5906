"""GPU: the in-state book's buffer is one for both device life cycles (capi_lifecycle.hip: book_alloc / book_release), so a book
left behind by one of them must not show through the other. One context goes from the immediate device life cycle to the pool
life cycle: the pool life cycle starts on an empty book, adopts the immediate one's on request (xivo_hip_pool_life_set_book),
and its first frame counts what the host life cycle counts from the same starting state."""
import numpy as np
import pytest

from xivo_amd import pcw, sequence
from xivo_amd import lib as L

pytestmark = pytest.mark.gpu

B, TRACKS = 2, 6
SIZES = dict(n_features=4, n_groups=3)
POOL = dict(SIZES, feature_init="subfilter", pool_max=8, anchor_max=4)


class _Recording(sequence.HipBackend):
    """the product backend that keeps the op lists the host life cycle sends"""

    def edit(self, ops):
        self.edits = getattr(self, "edits", []) + [np.array(ops, dtype=L.edit_dtype)]
        super().edit(ops)


def _tracks(cfg):
    """6 tracks per filter inside the image, depths inside (min_depth, max_depth)"""
    rng = np.random.default_rng(7)
    out = []
    for b in range(B):
        meas = np.stack([rng.uniform(40.0, cfg.cam["cols"] - 40.0, TRACKS), rng.uniform(40.0, cfg.cam["rows"] - 40.0, TRACKS),
                         rng.uniform(1.0, 3.0, TRACKS)], axis=1)
        assert (meas[:, 2] > cfg.min_depth).all() and (meas[:, 2] < cfg.max_depth).all()
        out.append((np.arange(100 * (b + 1), 100 * (b + 1) + TRACKS, dtype=np.int64), meas))
    return out


def _after_one_immediate_frame(tracks):
    """a context after one frame of the immediate device life cycle and its book (feat_id, feat_ref, group_refs); the life
    cycle is switched off and the pool configured"""
    cfg = sequence.SequenceConfig(lifecycle="device", tracks_max=16, **SIZES)
    sims = [pcw.TrajectorySim("lissajous", seed=900 + b) for b in range(B)]
    be = _Recording(cfg, B, sequence.initial_poses(cfg, sims), np.repeat(cfg.P_init()[None], B, axis=0))
    try:
        sequence.SequenceRunner(be, cfg, B).frame(None, tracks)
        book = be.life_book()
        be.ctx.life_config(0)
        be.cfg = sequence.SequenceConfig(**POOL)
        be.enable_pool()
    except Exception:
        be.close()
        raise
    return be, book


def test_pool_life_cycle_after_the_immediate_one(built):
    """B = 2, 4 feature slots, 3 group slots, 8 pool entries, 4 anchors, tracks_max = 16, 6 tracks per filter. After one frame of
    the immediate life cycle (4 features and a group entered per filter) the pool life cycle, configured on the same context,
    reads every slot, group and entry free; pool_life_set_book of the immediate book reads back as that book with group_refs
    rebuilt from the resident scene; a pool-life-cycle frame over the same tracks then returns OK and counts dropped, rejected
    and updates as the host life cycle does on a second context brought to the same state (dropped of the host: the
    REMOVE_FEATURE ops of its edit before the update)."""
    tracks = _tracks(sequence.SequenceConfig(**SIZES))
    D, A = _after_one_immediate_frame(tracks)
    H = None
    try:
        fid, fref, grefs = A
        assert (fid >= 0).sum() == B * SIZES["n_features"] and (grefs >= 0).sum() == B, "features and a group entered"
        cfg_d = sequence.SequenceConfig(pool_lifecycle="device", tracks_max=16, **POOL)
        D.cfg = cfg_d
        D.enable_device_pool_lifecycle()
        bk = D.pool_life_book()
        for name in ("feat_id", "feat_ref", "group_refs", "ent_id"):
            assert (bk[name] == -1).all(), name
        assert not bk["anc_used"].any()
        D.ctx.pool_life_set_book(fid)
        bk = D.pool_life_book()
        assert np.array_equal(bk["feat_id"], fid) and np.array_equal(bk["feat_ref"], fref)
        assert np.array_equal(bk["group_refs"], grefs)
        assert (bk["ent_id"] == -1).all() and not bk["anc_used"].any()

        # the host arm: the same frame on a second context (the same calls: the same state), its books set to A
        H, A_h = _after_one_immediate_frame(tracks)
        assert all(np.array_equal(x, y) for x, y in zip(A, A_h))
        assert D.covariance().tobytes() == H.covariance().tobytes()
        cfg_h = sequence.SequenceConfig(pool_lifecycle="host", **POOL)
        rh = sequence.SequenceRunner(H, cfg_h, B)
        for b, hb in enumerate(rh.books):
            hb.feat_id, hb.feat_ref, hb.group_refs = fid[b].tolist(), fref[b].tolist(), grefs[b].tolist()
            hb.id2slot = {i: j for j, i in enumerate(hb.feat_id) if i >= 0}
        H.edits = []
        rh.frame(None, tracks)
        host_dropped = int((H.edits[0]["kind"] == L.EDIT_REMOVE_FEATURE).sum())

        rd = sequence.SequenceRunner(D, cfg_d, B)
        rd.frame(None, tracks)   # (a refusal raises)
        st = D.pool_life_stats()
        got = dict(dropped=int(st["dropped"].sum()), rejected=int(st["rejected"].sum()), updates=int(st["updates"].sum()))
        want = dict(dropped=host_dropped, rejected=rh.n_rejected, updates=rh.n_updates)
        print("device", got, "host", want)
        assert got == want
        assert want["updates"] == B, "every filter had features in the state"
        bk = D.pool_life_book()
        for b, hb in enumerate(rh.books):
            assert bk["feat_id"][b].tolist() == hb.feat_id and bk["group_refs"][b].tolist() == hb.group_refs, b
            assert bk["ent_id"][b].tolist() == rh.pools[b].ent_id, b
    finally:
        D.close()
        if H is not None:
            H.close()
