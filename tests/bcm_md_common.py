"""What the committee-in-the-device-loop tests share: the two models of g12_bcm.npz on the 40-atom g5_big40 frame, built as
active_common.check_g12_bcm builds them, the committee rule of calculator_bcm.update_results in numpy, and a thermal start."""
import numpy as np

from helpers import load


def g12_posts(make_engine, keys=("a", "live")):
    """{key: PosteriorPotential} of the g12_bcm models on fresh engines, and the g5_big40 frame."""
    from autoforce_amd.model import Local
    from autoforce_amd.posterior import PosteriorPotential
    want, g = load("g12_bcm"), load("g5_big40")
    ptr = g["ind_ptr"]
    locs = [Local(int(z), g["ind_nbr_z"][ptr[q]:ptr[q + 1]], g["ind_nbr_r"][ptr[q]:ptr[q + 1]]) for q, z in enumerate(g["ind_z"])]
    posts = {}
    for key in keys:
        eng = make_engine()
        eng.set_inducing([locs[i] for i in want[f"{key}_idx"]])
        eng.set_weights(want[f"{key}_mu"], mean=dict(zip(want[f"{key}_mean_z"].tolist(), want[f"{key}_mean_w"].tolist())),
                        vscale=dict(zip(want[f"{key}_vscale_z"].tolist(), want[f"{key}_vscale"].tolist())), choli=want[f"{key}_choli"])
        eng.ridge = float(want[f"{key}_ridge"])
        posts[key] = PosteriorPotential(eng)
        posts[key].mean.weights.update(dict(zip(want[f"{key}_mean_z"].tolist(), want[f"{key}_mean_w"].tolist())))
    return posts, g


def g12_calculator(make_engine, members=True, **kw):
    """BCMActiveCalculator(live = "live", one frozen member "a" or none) without a teacher: it evaluates only (active is False)."""
    from autoforce_amd.calculator_bcm import BCMActiveCalculator
    posts, g = g12_posts(make_engine)
    kw.setdefault("logfile", None)
    return BCMActiveCalculator(covariance=posts["live"], kernel_model_dict={"a": posts["a"]} if members else {}, **kw), g


def thermal_velocities(numbers, temperature=300.0, seed=3):
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import MASS
    mass = np.array([MASS[int(z)] for z in numbers])[:, None]
    v = np.random.default_rng(seed).normal(size=(len(numbers), 3)) * np.sqrt(kB * temperature / mass)
    return v - (mass * v).sum(0) / mass.sum()


def committee_rule(outs):
    """calculator_bcm.update_results on the members' predict() dicts (the live model last): w, covmax, and the combined
    energy, forces, stress, beta_tot — sums accumulated in member order."""
    covmax = np.array([float(np.max(o["beta"])) for o in outs])
    w = weights_of(covmax)
    E = sum(a * o["energy"] for a, o in zip(w, outs))
    F = sum(a * o["forces"] for a, o in zip(w, outs))
    S = sum(a * o["stress"] for a, o in zip(w, outs))
    bt = outs[0]["beta"]
    for o in outs[1:]:
        bt = np.minimum(bt, o["beta"])
    return dict(w=w, covmax=covmax, energy=E, forces=F, stress=S, beta=bt)


def weights_of(covmax):
    with np.errstate(divide="ignore"):
        s = np.array([((-np.log(c) if c < 1.0 else 0.0) / c) if c > 0.0 else np.inf for c in covmax], float)
    w = np.isinf(s).astype(float) if np.isinf(s).any() else s
    if w.sum() <= 0.0:
        w = np.zeros(len(covmax))
        w[-1] = 1.0
    return w / w.sum()
