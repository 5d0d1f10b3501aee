"""Gates of the engine-vs-oracle comparisons that several GPU test modules share (test_parity_gpu.py,
test_solve_builds_gpu.py).  Plain helpers, no fixtures: every function asserts and returns what it measured."""
import numpy as np

from conftest import converged, rel_u0_err

TOL = 1e-4   # BASELINE.json north_star: "matching reference controls to 1e-4 rel"


def certify_converged(p, status, X, U, kink_wall_tol=None, ipopt_factor=1.0):
    """KKT certificate of the reference NLP (oracle/kkt_batch.py: multipliers re-fitted from the primal point alone, no solver
    involved) for EVERY instance of the batch `p` (nlp_batch.Batch) that `status` calls converged, at its own tolerance: 1e-8,
    or 1e-6 for an instance that ended at IPOPT's acceptable level (status 6 / 7).  Stationarity both relative to
    max(1, |grad f|_inf) and in IPOPT's own units (residual of the scaled problem / s_d, Waechter & Biegler eq. (5), (6)), with
    non-negative multipliers complementary to the tolerance in the units of IPOPT's criterion (the objective scaled by
    sf = 100 / |grad f(start)|_inf, computed from the NLP data alone); dynamics to rounding; no bound violated.
    kink_wall_tol (off by default): for an instance that ended on the d = 1 discontinuity (status 5 / 7) and misses the
    certificate with a wall candidate only where d^2 - 1 <= 1e-6, the certificate is repeated with that looser wall band
    (the other gates stay as they are).  ipopt_factor (1 by default): the bar of the IPOPT-units measure as a multiple of
    the tolerance.
    Returns dict(sel, cert, sf, tol) of the certified instances."""
    import kkt_batch as kb
    status = np.asarray(status)
    sel = np.nonzero(converged(status))[0]
    if sel.size == 0:
        return dict(sel=sel, cert=None, sf=np.zeros(0), tol=np.zeros(0))
    q = p.take(sel)
    sf = kb.objective_scale(q)
    tol_i = np.where(status[sel] >= 6, 1e-6, 1e-8)
    cert = kb.certify(q, X[sel], U[sel], eps_c=tol_i / sf, sf=sf)
    if kink_wall_tol is not None:
        kink = (status[sel] == 5) | (status[sel] == 7)
        redo = np.nonzero(kink & ((cert["stationarity"] > tol_i) | (cert["stationarity_ipopt"] > tol_i)))[0]
        if redo.size:
            r = kb.certify(q.take(redo), X[sel[redo]], U[sel[redo]], eps_c=tol_i[redo] / sf[redo], sf=sf[redo],
                           wall_tol=kink_wall_tol)
            for k in cert:
                cert[k][redo] = r[k]
    assert (cert["stationarity"] <= tol_i).all(), (cert["stationarity"].max(), sel[cert["stationarity"].argmax()])
    assert (cert["stationarity_ipopt"] <= ipopt_factor * tol_i).all(), \
        (cert["stationarity_ipopt"].max(), sel[cert["stationarity_ipopt"].argmax()])
    assert cert["feasibility"].max() <= 1e-10, cert["feasibility"].max()
    assert cert["bound_violation"].max() == 0.0, cert["bound_violation"].max()
    return dict(sel=sel, cert=cert, sf=sf, tol=tol_i)


def agreement(got, want):
    """What the fraction gates look at: converged on both sides, equal statuses, u0 error, equal iteration counts."""
    both = converged(got["status"]) & converged(want["status"])
    err = rel_u0_err(got["u0"], want["u0"])
    return dict(both=float(both.mean()), status=float((got["status"] == want["status"]).mean()),
                p99=float(np.percentile(err[both], 99)) if both.any() else 0.0,
                iters=float((got["iters"] == want["iters"])[both].mean()) if both.any() else 1.0,
                agree=float((err[both] <= TOL).mean()) if both.any() else 1.0, n_both=int(both.sum()))
