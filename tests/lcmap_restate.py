"""A numpy restatement of the resident landmark map (xivo_hip_lcmap_*): what becomes of an add record, which queries fill a
filter's match list, the gate of a match, whether the filter closes - and the rows, which are xivo_oracle.lc_jacobian_rows with
the stored point as the old feature's world point. Written from the header's text, not from the kernels; the host driver
(tests/lcmap_driver.cpp, the integer rules of lcmap_device.h) and the GPU tests are held against it."""
import numpy as np

import xivo_oracle as orc

ACCEPT, SKIPPED, POOR, DUP, FULL = range(5)
NONE, SHORT, CLOSED = range(3)
STATS = ("added", "dup", "full", "poor", "skipped", "queries", "matched", "surplus", "gated", "short_frames", "closed_frames")
_ADD_STAT = {ACCEPT: "added", SKIPPED: "skipped", POOR: "poor", DUP: "dup", FULL: "full"}


def is_poor(var, max_depth_var):
    return max_depth_var > 0.0 and var > max_depth_var


class MapRestate:
    """one filter's map"""

    def __init__(self, map_max, lc_max, min_matches):
        self.map_max, self.lc_max, self.min_matches = map_max, lc_max, min_matches
        self.keys, self.Xs = [], []
        self.stats = dict.fromkeys(STATS, 0)

    def add(self, recs):
        """recs: [(key, in_state, poor, Xs)] in order -> the outcome of each"""
        out = []
        for key, in_state, poor, Xs in recs:
            if not in_state or key < 0:
                d = SKIPPED
            elif poor:
                d = POOR
            elif key in self.keys:
                d = DUP                                   # the first estimate stays (merge_features = false)
            elif len(self.keys) >= self.map_max:
                d = FULL                                  # nothing is evicted
            else:
                d = ACCEPT
                self.keys.append(key); self.Xs.append(None if Xs is None else np.array(Xs, dtype=np.float64))
            self.stats[_ADD_STAT[d]] += 1
            out.append(d)
        return out

    def match(self, qkeys):
        """-> (slot of every query: list position, -1 no match, -2 surplus; the list [(query, entry)])"""
        slots, lst = [], []
        for q, key in enumerate(qkeys):
            if key < 0 or key not in self.keys:
                slots.append(-1)
            elif len(lst) < self.lc_max:
                slots.append(len(lst)); lst.append((q, self.keys.index(key)))
            else:
                slots.append(-2)
        self.stats["queries"] += len(qkeys); self.stats["matched"] += len(lst)
        self.stats["surplus"] += sum(s == -2 for s in slots)
        return slots, lst

    def decide(self, kept):
        """kept: the gate's answer of every filled list position -> (frame, neutral flag of all lc_max pairs)"""
        n, k = len(kept), int(sum(bool(v) for v in kept))
        frame = CLOSED if (k >= self.min_matches and k > 0) else (SHORT if n > 0 else NONE)
        neutral = [frame != CLOSED or m >= n or not kept[m] for m in range(self.lc_max)]
        self.stats["gated"] += n - k
        self.stats["short_frames"] += frame == SHORT; self.stats["closed_frames"] += frame == CLOSED
        return frame, neutral


def world_point(x, gR, gT, Rbc, Tbc, invdepth=False):
    """Feature::Xs(gbc) of an in-state feature anchored in the group (gR, gT)"""
    return orc.feature_xs(np.asarray(x), np.asarray(gR), np.asarray(gT), np.asarray(Rbc), np.asarray(Tbc), invdepth)


def rows(matches, Rbc, Tbc, cam, lay, lc_max, Rlc):
    """matches: [dict(Xs, Rsb, Tsb: the observing pose, g_sind: its group slot or -1 for the body pose, xp)] -> (H [2 lc_max, N],
    inn, diagR) of the filled positions, the others neutral. The stored point enters the oracle as a feature at unit depth on the
    axis of a camera whose anchor has identity rotation; body-observed pairs are built in group slot 0 and their group block
    moved to columns 0..5 (the body and a group share the retraction)."""
    H = np.zeros((2 * lc_max, lay.N)); inn = np.zeros(2 * lc_max); dR = np.ones(2 * lc_max)
    e3 = np.array([0.0, 0.0, 1.0])
    for i, m in enumerate(matches):
        Tsbr = np.asarray(m["Xs"]) - (Rbc @ e3 + Tbc)
        g = int(m["g_sind"])
        mm = dict(x=np.zeros(3), Rsbr=np.eye(3), Tsbr=Tsbr, Rsb=m["Rsb"], Tsb=m["Tsb"], g_sind=max(g, 0), xp=m["xp"])
        Hi, ii = orc.lc_jacobian_rows([mm], Rbc, Tbc, cam, lay)
        if g < 0:
            gb = lay.group_begin
            blk = Hi[:, gb:gb + 6].copy(); Hi[:, gb:gb + 6] = 0.0; Hi[:, 0:6] = blk
        H[2 * i:2 * i + 2] = Hi; inn[2 * i:2 * i + 2] = ii; dR[2 * i:2 * i + 2] = Rlc
    return H, inn, dR


def gamma(Hi, P, r, Rlc):
    """r^T (H_i P H_i^T + Rlc I)^-1 r of one pair; None (the device shows -1) where S has a non-positive pivot or the value is
    not finite - a NaN or inf pixel or stored point"""
    S = Hi @ P @ Hi.T + Rlc * np.eye(2)
    if not (S[0, 0] > 0 and S[1, 1] - S[1, 0] ** 2 / S[0, 0] > 0):
        return None
    with np.errstate(all="ignore"):
        g = float(r @ np.linalg.solve(S, r))
    return g if np.isfinite(g) else None


def kept(g, chi2):
    """the gate of one match on gamma() (lcmap_kept): no pivot or no finite gamma is never kept, whatever chi2 is; chi2 = 0 is no
    gate, equality keeps"""
    return g is not None and bool(np.isfinite(g)) and not (chi2 > 0.0 and g > chi2)


def neutralise(H, inn, dR, neutral):
    H, inn, dR = H.copy(), inn.copy(), dR.copy()
    for m, nt in enumerate(neutral):
        if nt:
            H[2 * m:2 * m + 2] = 0.0; inn[2 * m:2 * m + 2] = 0.0; dR[2 * m:2 * m + 2] = 1.0
    return H, inn, dR
