"""The checker of the rejection log (learn_network(track_rejections=True), fw_set_track_rejections): the driver of
tests/hiton_exact_ref.py with the rejection branch of update_sig_result! (src/hiton.jl:71-76) added.

When a candidate is tested against a non-empty accepted list and the returned test is not significant, the record
rej[T][candidate] = (phase, Zs, stat, pval, df, suff_power, num_tests, frac) is kept, straight from Oracle.test_subsets (the first
non-significant test in the reference's enumeration order, src/tests.jl:281-346).  hiton_exact_ref is imported and wrapped, not
edited: its phase routine is swapped for the one below while learn() runs."""
import math

from tests import hiton_exact_ref as H
from tests.hiton_exact_ref import make_oracles  # noqa: F401


def _make_phase(rej):
    def _phase(orc, T, cands, phase, wl, support, P, fast_elim, counter):
        acc = list(cands) if phase == "E" else []
        out = {}
        for cand in cands:
            if cand in wl:  # hiton.jl:20-30
                acc.append(cand)
                out[cand] = (math.nan, math.nan)
                continue
            if phase == "E":  # :134-136
                acc = [v for v in acc if v != cand]
            r = orc.test_subsets(T, cand, acc, max_k=P["max_k"], alpha=P["alpha"], hps=P["hps"], n_obs_min=P["n_obs_min"],
                                 max_tests=P["max_tests"])
            if r["num_tests"] > 0:
                counter[0] += r["num_tests"]
            if not acc:  # :57-59
                acc.append(cand)
                out[cand] = support[cand]
            elif r["pval"] < P["alpha"] and r["suff_power"]:  # :61-63
                acc.append(cand)
                out[cand] = (r["stat"], r["pval"])
            else:  # :67-76
                assert cand not in rej.setdefault(T, {}), "a candidate is rejected at most once per target"
                rej[T][cand] = dict(phase=0 if phase == "I" else 1, Zs=tuple(r["Zs"]), stat=r["stat"], pval=r["pval"], df=r["df"],
                                    suff_power=bool(r["suff_power"]), num_tests=r["num_tests"], frac=r["frac"], pool=tuple(acc))
                if phase == "E" and not fast_elim:
                    acc.append(cand)
        return out
    return _phase


def learn(orc, discrete, **kw):
    """H.learn(...) plus "rejections" = {target: {candidate: record}} (0-based ids; record["pool"]: the accepted list the
    candidate was tested against)."""
    rej = {}
    saved = H._phase
    H._phase = _make_phase(rej)
    try:
        net = H.learn(orc, discrete, **kw)
    finally:
        H._phase = saved
    net["rejections"] = rej
    return net
