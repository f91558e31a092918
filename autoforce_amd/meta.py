"""Metadynamics: the bias potential of the reference's theforce/calculator/meta.py (Meta over theforce/analysis/kde.py's
Gaussian_kde; its example is examples/meta-dyn/md.py) for ActiveCalculator(meta=) and the MD loops.

    meta = Meta(Catvar(Posvar(1, select=3), Distance(0, 5)), sigma=0.1, w=0.01, tem=None)
    calc = ActiveCalculator(..., meta=meta)
    for _ in calc.run_md(atoms, steps, 600.0): ...       # the bias runs inside the device loop (SGPRModel.md_meta)

A Meta adds V(cv) = w kde(cv) — with tem the well-tempered log(1 + w kde gamma) / gamma, gamma = 1 / (kB tem) — to the energy,
-dV/dx to the forces and -(1/V_cell) sum_i x_i (x) F_i to the stress of every calculate(), as the reference's post_calculate does
with op="+=" (calculator/active.py:510-516, :557-580), and update() deposits a hill where the last bias was evaluated (the
reference: dyn.attach(meta.update)) and appends the CV to meta.hist.  workloads.meta_bias is the definition of the built-in
collective variables Distance, Posvar, Qlvar and Catvar; for these the device MD loop evaluates the bias itself
(device_spec()).
Any other colvar — a function (numbers, xyz, cell, pbc, nl) -> 1-d torch tensor of xyz, the reference's interface — is
differentiated with torch.autograd on the host path.
"""
import numpy as np


class Distance:
    """|x_j - x_i| of the raw coordinates (no minimum image): one dimension — the reference docstring's example colvar."""
    dim = 1

    def __init__(self, i, j):
        self.i, self.j = int(i), int(j)

    def spec(self):
        return [("distance", self.i, self.j)]

    def __call__(self, numbers, xyz, cell=None, pbc=None, nl=None):
        d = np.asarray(xyz, float)[self.j] - np.asarray(xyz, float)[self.i]
        return np.array([np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])])


class Posvar:
    """The reference's Posvar: x_index - (1/n) sum_{k in sel, k != index} x_k, sel all atoms or the atoms of species `select`,
    n = |sel| — the index atom counts in n where it is in sel (the reference's mean over a * p with a[index] = 0).  Three
    dimensions, raw coordinates."""
    dim = 3

    def __init__(self, index, select=None):
        self.index, self.select = int(index), (None if select is None else int(select))

    def spec(self):
        return [("posvar", self.index, self.select)]

    def __call__(self, numbers, xyz, cell=None, pbc=None, nl=None):
        x = np.asarray(xyz, float)
        sel = np.ones(len(x), bool) if self.select is None else (np.asarray(numbers) == self.select)
        a = sel.copy()
        a[self.index] = False
        return x[self.index] - x[a].sum(axis=0) / float(sel.sum())


class Qlvar:
    """The reference's Qlvar(i, j, index=None, cutoff=4.0, l=[6]): the Steinhardt bond-order parameters Q_l of atom `index` (of
    species i; None: the first atom with numbers == i, resolved at the first use; RuntimeError where numbers[index] != i) over
    its neighbours t of species j with r_t < cutoff, r_t = x_j - x_index + shift.cell:
        w_t = (1 - r_t / cutoff)^2, W = sum w_t, q_lm = sum_t w_t Y_lm(r^_t) / W, Q_l = sqrt(4 pi / (2l + 1) sum_m |q_lm|^2)
    evaluated by the addition theorem, Q_l^2 = sum_{t,t'} w_t w_t' P_l(r^_t . r^_t') / W^2 (workloads.ql_dim is the definition:
    no Y_lm, no pole on the z axis, 0 <= l <= 12).  len(l) dimensions, in the order of l.  The device loop reads the model's own
    neighbour list, which ends at the model's rc: cutoff <= rc is required (Meta.bias refuses a larger one).
      Like the reference's Ylm, the whole environment is sheared by 1e-2 when a selected neighbour lies within 1e-2 of the z axis
    (workloads.ql_rows): Q_l then differs from the unsheared value by up to a few 1e-5, as the reference's does.
      Where this departs from the reference: an empty environment gives Q_l = 0 with zero gradient (there: NaN, 0 / 0), and
    where Q_l = 0 the gradient is 0 (there: NaN, which nan_to_num turns into 0)."""

    def __init__(self, i, j, index=None, cutoff=4.0, l=[6]):
        self.i, self.j, self.index = int(i), int(j), (None if index is None else int(index))
        self.cutoff, self.l = float(cutoff), tuple(int(v) for v in l)
        self.dim = len(self.l)

    def resolve(self, numbers):
        numbers = np.asarray(numbers)
        if self.index is None:
            found = np.where(numbers == self.i)[0]
            if not len(found):
                raise RuntimeError(f"Qlvar: no atom with numbers == {self.i}")
            self.index = int(found[0])
        if numbers[self.index] != self.i:
            raise RuntimeError(f"numbers[{self.index}] != {self.i}")
        return self.index

    def spec(self):
        return [("qlvar", self.index, self.j, self.cutoff, self.l)]

    def __call__(self, numbers, xyz, cell, pbc, nl=None):
        from .workloads import ql_dim, ql_environment, ql_rows
        idx = self.resolve(numbers)
        _, _, r, ln = ql_environment(numbers, xyz, cell, pbc, idx, self.j, self.cutoff, nl=nl)
        rows = ql_rows(r, ln, self.cutoff)
        return np.array([ql_dim(l, *rows)[0] for l in self.l])


class Catvar:
    """Components concatenated (the reference's Catvar)."""

    def __init__(self, *var):
        self.var = var

    def spec(self):
        out = []
        for v in self.var:
            s = v.spec() if hasattr(v, "spec") else None
            if s is None:
                return None
            out += s
        return out

    def resolve(self, numbers):
        for v in self.var:
            if hasattr(v, "resolve"):
                v.resolve(numbers)

    def __call__(self, *args):
        return np.concatenate([np.asarray(v(*args), float).reshape(-1) for v in self.var])


class Meta:
    """Meta(colvar, sigma=0.1, w=0.01, tem=None): the reference's constructor — it opens meta.hist with the header line
    `# sigma` — plus pace (configuration n deposits when n % pace == 0; the reference: 1), hist (the file; None: none) and
    merge (a chunk length: the hills are merged by bin, chunk after chunk, workloads.meta_density(merge=) — the cost of the bias
    then grows with the bins visited, not with time; the device loop takes it as SGPRModel.md_meta(merge=); None: every hill on
    its own)."""

    def __init__(self, colvar, sigma=0.1, w=0.01, tem=None, pace=1, hist="meta.hist", merge=None):
        self.colvar, self.sigma, self.w, self.tem, self.pace, self.hist = colvar, sigma, float(w), tem, int(pace), hist
        self.merge = None if merge is None else int(merge)
        if self.merge is not None and self.merge < 1:
            raise ValueError(f"Meta: merge is a chunk length >= 1 or None, not {merge}")
        self.species = None   # the model's species table: the order in which a posvar's mean is summed (None: sorted numbers)
        self.rc = None        # the model's cutoff: a Qlvar reads the model's list (ActiveCalculator and run_md set it)
        self.hills = []     # CV values of the deposits, in order
        self.n = 0          # configurations update() has seen
        self._cv = None
        self.energy = 0.0   # the bias of the last evaluation
        if self.hist:
            with open(self.hist, "w") as hst:
                hst.write(f"# {sigma}\n")

    def device_spec(self):
        """The components as SGPRModel.md_meta takes them, or None when one is not built in (Distance, Posvar, Qlvar, Catvar
        of them; at most 4 components and 6 dimensions).  A Qlvar(index=None) stands with index None until resolve(numbers)."""
        from .workloads import meta_cv_dim
        s = self.colvar.spec() if hasattr(self.colvar, "spec") else None
        if not s or len(s) > 4 or meta_cv_dim(s) > 6:
            return None
        return s

    def resolve(self, numbers):
        """Fixes the atom of every Qlvar(index=None) (the first of its species) and checks the species at the index."""
        if hasattr(self.colvar, "resolve"):
            self.colvar.resolve(numbers)

    def hills_array(self, D=None):
        return np.asarray(self.hills, float).reshape(len(self.hills), -1) if self.hills else np.zeros((0, D or 0))

    def histogram(self):
        """(centres [T, D], counts [T]) of the hills held, merged by bin — the reference's Gaussian_kde.histogram() — by the rule
        of workloads.meta_table: with merge, the rows below the last whole chunk (what the merged bias sums as entries, and what
        SGPRModel.md_meta_table() returns); without, all of them."""
        from .workloads import meta_table
        H = self.hills_array()
        if not len(H):
            return np.zeros((0, H.shape[1])), np.zeros(0)
        sg = np.asarray(self.sigma, float).reshape(-1)
        centres, _, counts, _ = meta_table(H, sg if len(sg) > 1 else sg[0], self.merge or 1)
        return centres, counts

    def bias(self, positions, cell, numbers=None, pbc=None, rc=None):
        """(V, forces [N, 3], stress [6]) of the bias at this configuration with the hills deposited so far; the CV is kept
        for update().  pbc and rc (the model's cutoff; default: self.rc): what a Qlvar needs."""
        from .workloads import meta_bias
        x = np.asarray(positions, float)
        numbers = np.zeros(len(x), int) if numbers is None else np.asarray(numbers)
        self.resolve(numbers)
        spec = self.device_spec()
        if spec is not None:
            kw = dict(pbc=pbc, rc=self.rc if rc is None else rc) if any(c[0] == "qlvar" for c in spec) else {}
            out = meta_bias(spec, self.sigma, self.w, numbers, x, cell, self.hills_array(), tem=self.tem, species=self.species, merge=self.merge, **kw)
            self._cv, self.energy, self.margin = out["cv"], out["energy"], out["margin"]
            return out["energy"], out["forces"], out["stress"]
        return self._bias_autograd(numbers, x, cell)

    def _bias_autograd(self, numbers, x, cell):
        """A colvar that is not built in: the reference's interface, a function of torch tensors; dV/dx by autograd, the
        density by workloads.meta_density on the CV itself."""
        import torch
        from .workloads import meta_density
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        cv = self.colvar(torch.as_tensor(np.asarray(numbers)), xt, torch.tensor(np.asarray(cell, float).reshape(3, 3)), None, None).reshape(-1)
        c = cv.detach().numpy()
        V, g, _ = meta_density(c, self.sigma, self.w, self.hills_array(len(c)), tem=self.tem, merge=self.merge)
        (gx,) = torch.autograd.grad(cv, xt, torch.tensor(g), allow_unused=True)
        F = np.zeros_like(x) if gx is None else -np.nan_to_num(gx.numpy())
        vol = abs(float(np.linalg.det(np.asarray(cell, float).reshape(3, 3))))
        vol = vol if vol > 0.0 else -2.0
        stress = (-(x[:, :, None] * F[:, None, :]).sum(axis=0) / vol).reshape(9)[[0, 4, 8, 5, 2, 1]]
        self._cv, self.energy, self.margin = c, float(V), None
        return float(V), F, stress

    def _write(self, cv):
        if self.hist:
            with open(self.hist, "a") as hst:
                for f in cv:
                    hst.write(f" {float(f)}")
                hst.write("\n")

    def update(self):
        """Called once per configuration behind its bias(): deposits its CV when its index is a multiple of pace."""
        if self._cv is None:
            return
        if self.n % self.pace == 0:
            self.hills.append(np.array(self._cv, float))
            self._write(self._cv)
        self.n += 1

    def absorb(self, cv_rows, n):
        """Hills the device loop deposited (SGPRModel.md_meta_hills), mirrored: calculate() at a halt sees the same bias; n:
        the configurations the loop has seen."""
        for cv in np.asarray(cv_rows, float):
            self.hills.append(np.array(cv))
            self._write(cv)
        self.n = int(n)

    def __call__(self, calc):
        """The calculator's hook (the reference's Meta.__call__): the bias energy of calc.atoms; post_calculate adds energy,
        forces and stress to calc.results."""
        at = calc.atoms
        eng = getattr(calc, "engine", None)
        V, F, S = self.bias(at.positions, getattr(at.cell, "array", at.cell), at.numbers, pbc=at.pbc, rc=getattr(eng, "cutoff", None))
        self._last = (V, F, S)
        return np.array([V]), {"op": "+=", "is_meta": True}
