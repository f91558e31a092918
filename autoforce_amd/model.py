"""Host-side mirror of the reference's model objects for the SGPR predict/solve hot path.

  Local      <- theforce/descriptor/atoms.py:36-55   (one local chemical environment, LCE)
  SGPRModel  <- theforce/regression/gppotential.py:453-1175 PosteriorPotential state
               (X, M, mu, choli, ridge, _vscale, mean) + the default kernel of
               theforce/calculator/active.py:28-38 (SeSoapKernel(lmax,nmax,exponent,cutoff,
               radii=DefaultRadii())).
All numerics run in libsgpr_hip.so (HIP, gfx950) through the C ABI; this file only marshals.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, f64, i32, i64, ptr


class Local:
    """An LCE: central atomic number, neighbour numbers `b` and displacement vectors `r`
    (= x_j - x_i + off.cell), as theforce/descriptor/atoms.py:36-55 (`number`, `_b`, `_r`)."""

    def __init__(self, number, b, r):
        self.number = int(number)
        self._b = i32(b).reshape(-1)
        self._r = f64(r).reshape(-1, 3)
        if len(self._b) != len(self._r):
            raise ValueError("Local: len(b) != len(r)")

    def __repr__(self):
        return f"Local(Z={self.number}, nn={len(self._b)})"


def _attach(code):
    """check() for the attach functions of the device loop: what the loop does not serve (SGPR_E_UNSUPPORTED) is a
    NotImplementedError — the host loop around calculate() serves it."""
    try:
        check(code)
    except _lib.SgprError as e:
        if e.code == -6:   # SGPR_E_UNSUPPORTED
            raise NotImplementedError(str(e)) from None
        raise


def default_radii(species):
    """DefaultRadii (theforce/descriptor/sesoap.py:84-99): 0.5 for H, else 1.0."""
    return np.array([0.5 if int(z) == 1 else 1.0 for z in species])


def recorded_indices(t0, done, code, every):
    """The trajectory indices of the frames that stand behind an md_run call (sgpr_md_frame_count's rule, for a caller's own
    bookkeeping): the call began at configuration t0, `done` rows came back with halt code `code`, every `every`-th
    configuration was recorded.  The rows' evaluations t0 ... t0 + done - 1 stand — an overflow (2) has left the halting one out
    of `done` already, a converged relaxation (3) keeps its last — less the last one when the covloss gate fired (1): the next
    call evaluates and records that configuration again."""
    if not every:
        return []
    last = t0 + done - (1 if code == 1 else 0)
    return [n for n in range(-(-t0 // every) * every, last, every)]


class SGPRModel:
    def __init__(self, lmax=3, nmax=3, exponent=4, cutoff=6.0, species=None, radii=None, device=0,
                 unknown_species="error", lone_weight=1):
        """unknown_species: "error" (default) or "ignore" — atoms and LCE neighbours whose atomic number is
        not in `species` are invisible, as in the reference's fixed-species kernels
        (descriptor/sesoap.py:343-346, similarity/heterosoap.py:37-71).
        lone_weight: k(x, x') of two lone atoms (no neighbour inside the cutoff) of one species.  The reference adds
        that term once per kernel OBJECT (similarity/similarity.py:38-40, :94-103) and sums the kernels
        (regression/gppotential.py:63-84): 1 for the wildcard SeSoapKernel, len(species) for the list of fixed-species
        kernels that `kernel_kw={'species': [...]}` builds (calculator/active.py:31-38)."""
        if species is None or len(species) == 0:
            raise ValueError("SGPRModel needs the species table (atomic numbers the model may meet)")
        self.lmax, self.nmax, self.exponent, self.cutoff = int(lmax), int(nmax), float(exponent), float(cutoff)
        self.species = [int(z) for z in species]
        self.radii = default_radii(self.species) if radii is None else f64(radii)
        self.device = int(device)
        self._h = C.c_void_p()
        lib = _lib.load()
        check(lib.sgpr_create(self.lmax, self.nmax, self.exponent, self.cutoff, len(self.species),
                              ptr(i32(self.species)), ptr(f64(self.radii)), self.device, C.byref(self._h)))
        self.unknown_species = unknown_species
        if unknown_species == "ignore":
            check(lib.sgpr_set_option(self._h, b"ignore_unknown_species", 1))
        elif unknown_species != "error":
            raise ValueError("unknown_species must be 'error' or 'ignore'")
        self.lone_weight = int(lone_weight)
        if self.lone_weight != 1:
            check(lib.sgpr_set_option(self._h, b"lone_atom_weight", self.lone_weight))
        self.X = []
        self.mu = None
        self._choli, self._choli_on_device = None, False
        self.ridge = 0.0
        self.sigma = None
        self.mean = {z: 0.0 for z in self.species}  # AutoMean weights (gppotential.py:200-231)
        self._vscale = {}
        self.generation = 0   # counts the frames the device evaluated (predict, training rows): whoever caches
                              # something about "the last frame" (calc.cov) can tell when it moved on
        self._pv = None       # predict_view's per-system cache
        self.comm_world = 1   # > 1 once an RCCL communicator is attached (comm_init)
        self.peer_world = 1   # > 1 once the library's own exchange is attached (peer_attach)

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.load().sgpr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def solve_info(self):
        """Route of the last data_solve / data_factor and tile forms of the last step (sgpr_solve_info):
        'stage1=...; kmm_blocks=a/b; step=...; rows=...'."""
        buf = C.create_string_buffer(512)
        check(_lib.load().sgpr_solve_info(self._h, buf, 512))
        return buf.value.decode()

    def list_rebuilds(self):
        """How many steps of this handle rebuilt the Verlet candidate lists so far (the others filtered the kept
        candidates: descriptor.hip)."""
        n = C.c_int64(0)
        check(_lib.load().sgpr_get_list_rebuilds(self._h, C.addressof(n)))
        return int(n.value)

    # ------------------------------------------------------------------ multi-GPU (one process per GPU)
    @staticmethod
    def comm_unique_id():
        """ncclUniqueId bytes (rank 0 creates them; the host passes them to the other ranks)."""
        buf = C.create_string_buffer(128)
        check(_lib.load().sgpr_comm_unique_id(C.addressof(buf)))
        return buf.raw

    def comm_init(self, uid, rank, world):
        """Attach an RCCL communicator (collective over all ranks): from now on a sharded predict() /
        sgpr_step_dev ends with ONE all-reduce of the packed buffer on the step's stream and returns
        totals (the reference's four MPI collectives, calculator/active.py:562,601,602,777)."""
        buf = C.create_string_buffer(bytes(uid), 128)
        check(_lib.load().sgpr_comm_init(self._h, C.addressof(buf), int(rank), int(world)))
        self.comm_world = int(world)

    def comm_destroy(self):
        check(_lib.load().sgpr_comm_destroy(self._h))
        self.comm_world = 1

    PEER_HANDLE_BYTES = 128

    def peer_export(self, rank, world, capacity):
        """This rank's receive buffers of the library's own exchange (hipIpc all-gather + local sum in rank order,
        include/sgpr_hip.h): `capacity` doubles per source rank (>= 7 N + 11 for frames of N atoms).  Returns the bytes
        every peer needs for peer_attach."""
        buf = C.create_string_buffer(self.PEER_HANDLE_BYTES)
        check(_lib.load().sgpr_peer_export(self._h, int(rank), int(world), int(capacity), C.addressof(buf)))
        return buf.raw

    def peer_attach(self, handles):
        """handles: the peer_export bytes of ALL ranks in rank order.  From now on sharded predict() / step / md_run
        combine the ranks' partial sums through this exchange: the same bits on every rank, independent of the number of
        ranks (the reference's collectives: calculator/active.py:562,600-602,770-777)."""
        blob = b"".join(bytes(x) for x in handles)
        buf = C.create_string_buffer(blob, len(blob))
        check(_lib.load().sgpr_peer_attach(self._h, C.addressof(buf)))
        self.peer_world = self.comm_world = len(handles)   # (comm_world: "the library combines the ranks itself")

    def peer_selftest(self, rank, world):
        """One small exchange with a known answer (every rank contributes rank + 1 in eight doubles): True when the sum came
        back on this rank.  The hosts call it right after peer_attach and agree on the outcome before they rely on the
        exchange (a rank whose stores are not seen by a peer would otherwise surface as a time-out in the first step)."""
        import torch
        buf = torch.full((8,), float(rank + 1), dtype=torch.float64, device=f"cuda:{self.device}")
        lib = _lib.load()
        try:
            check(lib.sgpr_comm_allreduce(self._h, buf.data_ptr(), 8, 0, None))
            check(lib.sgpr_sync_check(self._h, None))
        except _lib.SgprError:
            return False
        return bool((buf.cpu().numpy() == world * (world + 1) / 2).all())

    def peer_destroy(self):
        check(_lib.load().sgpr_peer_destroy(self._h))
        self.peer_world = self.comm_world = 1

    def scratch(self):
        """A second, empty model with the same kernel on the same device (used for one-off
        K(atoms, atoms) evaluations that must not disturb this model's inducing set)."""
        return SGPRModel(self.lmax, self.nmax, self.exponent, self.cutoff, species=self.species, radii=self.radii,
                         device=self.device, unknown_species=self.unknown_species, lone_weight=self.lone_weight)

    def with_species(self, species):
        """The same model over another species table (same kernel, inducing LCEs, weights): how the
        wildcard kernel of the reference (calculator/active.py:28-38, a 120-wide sparse table) is
        served by a dense table — it is re-laid-out when a new species turns up.  Descriptor blocks
        of absent species are zero, so every kernel value, mu and choli stay what they were."""
        # species already in the table keep their length unit (a model built with custom radii must not fall back
        # to the defaults on the first re-layout: the kernel would change under mu and choli); new ones get the
        # default (descriptor/sesoap.py:84-99)
        have = {int(z): float(r) for z, r in zip(self.species, self.radii)}
        radii = [have.get(int(z), float(default_radii([z])[0])) for z in species]
        new = SGPRModel(self.lmax, self.nmax, self.exponent, self.cutoff, species=species, radii=radii,
                        device=self.device, unknown_species=self.unknown_species, lone_weight=self.lone_weight)
        new.mean.update(self.mean)
        new._vscale = dict(self._vscale)
        if self.X:
            new.set_inducing(self.X)
            if self.mu is not None:
                new.set_weights(self.mu, mean=self.mean, vscale=self._vscale or None, choli=self.choli)
        new.ridge, new.sigma = self.ridge, self.sigma
        return new

    # ------------------------------------------------------------------ inducing set
    def set_inducing(self, X):
        """model.X = inducing LCEs; builds descriptors and K_mm on the device
        (gppotential.py:484-509 set_data: self.M = kern(X, X))."""
        X = list(X)
        m = len(X)
        zc = i32([x.number for x in X])
        nptr = i64(np.concatenate([[0], np.cumsum([len(x._b) for x in X])]))
        nz = i32(np.concatenate([x._b for x in X] + [np.zeros(0, np.int32)]))
        nr = f64(np.concatenate([x._r for x in X] + [np.zeros((0, 3))]))
        self.generation += 1
        check(_lib.load().sgpr_set_inducing(self._h, m, ptr(zc), ptr(nptr), ptr(nz), ptr(nr)))
        self.X = X  # (after the device accepted it: on an error host and device lists still agree)
        self.mu = None
        self.choli = None

    @property
    def choli(self):
        """L^-1 of the K_mm factor, [m, m].  A device solve leaves it on the device; it is downloaded when somebody
        looks (leakage, model files), not at every refit."""
        if self._choli is None and self._choli_on_device and self.m:
            out = np.zeros((self.m, self.m))
            check(_lib.load().sgpr_get_choli(self._h, ptr(out)))
            self._choli = out
        return self._choli

    @choli.setter
    def choli(self, value):
        self._choli, self._choli_on_device = value, False

    def _weights_dropped(self):
        self.mu = None
        self.choli = None

    def add_inducing(self, loc):
        """Append one LCE (PosteriorPotential.add_inducing, gppotential.py:745-772, without the
        data columns — those are `kernel_columns`)."""
        self.generation += 1  # (stored data frames are re-bound for their new column)
        check(_lib.load().sgpr_add_inducing(self._h, loc.number, len(loc._b), ptr(loc._b), ptr(loc._r)))
        self.X.append(loc)
        self._weights_dropped()

    def remove_inducing(self, index=-1):
        """pop_1inducing / popfirst_1inducing (gppotential.py:782-813)."""
        check(_lib.load().sgpr_remove_inducing(self._h, int(index)))
        del self.X[index]
        self._weights_dropped()

    def select_inducing(self, indices):
        """Keep `indices` in the given order (gppotential.py:1037-1046)."""
        idx = i32(indices)
        check(_lib.load().sgpr_select_inducing(self._h, len(idx), ptr(idx)))
        self.X = [self.X[int(j)] for j in idx]
        self._weights_dropped()

    def kernel_local(self, loc):
        """(k(loc, X)[m], k(loc, loc)) for an LCE outside the inducing set (active.py:806-818)."""
        k = np.zeros(self.m)
        kxx = C.c_double(0)
        check(_lib.load().sgpr_kernel_local(self._h, loc.number, len(loc._b), ptr(loc._b), ptr(loc._r), ptr(k),
                                            C.addressof(kxx)))
        return k, kxx.value

    @property
    def m(self):
        return len(self.X)

    @property
    def M(self):
        out = np.zeros((self.m, self.m))
        check(_lib.load().sgpr_get_kmm(self._h, ptr(out)))
        return out

    @property
    def M_diag(self):
        out = np.zeros(self.m)
        check(_lib.load().sgpr_get_kmm_diag(self._h, ptr(out)))
        return out

    @property
    def M_rowsum(self):
        """K_mm.sum(axis=1), caller order, summed on the device in numpy's own order (bit for bit `self.M.sum(axis=1)`)."""
        out = np.zeros(self.m)
        check(_lib.load().sgpr_get_kmm_rowsum(self._h, ptr(out)))
        return out

    @property
    def dims(self):
        out = np.zeros(8, np.int32)
        check(_lib.load().sgpr_get_dims(self._h, ptr(out)))
        return dict(m=int(out[0]), S=int(out[1]), D=int(out[2]), Dc=int(out[3]), maxnn=int(out[4]), N=int(out[5]),
                    nn_max=int(out[6]), Dpad=int(out[7]))

    def inducing_descriptors(self):
        S, D = len(self.species), (self.nmax + 1) ** 2 * (self.lmax + 1)
        out = np.zeros((self.m, S, S, D))
        check(_lib.load().sgpr_get_inducing_descriptors(self._h, ptr(out)))
        return out

    # ------------------------------------------------------------------ weights
    def _table(self, d, default):
        return f64([d.get(z, default) if d is not None else default for z in self.species])

    def set_weights(self, mu, mean=None, vscale=None, choli=None):
        """Install mu / AutoMean weights / _vscale / choli (gppotential.py:548-605,644-649)."""
        self.mu = f64(mu).copy()
        if mean is not None:
            self.mean.update({int(z): float(w) for z, w in mean.items()})
        if vscale is not None:
            self._vscale = {int(z): float(v) for z, v in vscale.items()}
        self.choli = None if choli is None else f64(choli).copy()
        vs = f64([self._vscale.get(z, np.inf) for z in self.species]) if self._vscale else None
        check(_lib.load().sgpr_set_weights(self._h, ptr(self.mu), ptr(self._table(self.mean, 0.0)), ptr(vs),
                                           ptr(self._choli)))

    def commit_weights(self, mean=None):
        """The tail of make_munu after a device solve: mu and choli are already installed on the device, only the
        AutoMean weights follow (_vscale is what make_vscale just computed)."""
        if mean is not None:
            self.mean.update({int(z): float(w) for z, w in mean.items()})
        check(_lib.load().sgpr_set_mean(self._h, ptr(self._table(self.mean, 0.0)), None))

    def snapshot_weights(self):
        """What a rejected trial has to put back (see restore_weights)."""
        return dict(mu=None if self.mu is None else self.mu.copy(), ridge=self.ridge, sigma=self.sigma,
                    vscale=dict(self._vscale), mean=dict(self.mean))

    def restore_weights(self, snap):
        """After the pop that ends a rejected trial: the weights saved before it, instead of a refit that would
        reproduce them (gppotential.py:898-982)."""
        check(_lib.load().sgpr_restore_weights(self._h, ptr(f64(snap["mu"]))))
        self.mu = snap["mu"].copy()
        self.ridge, self.sigma = snap["ridge"], snap["sigma"]
        self._vscale = dict(snap["vscale"])
        self.mean.update(snap["mean"])
        self._choli, self._choli_on_device = None, True
        vs = f64([self._vscale.get(z, np.inf) for z in self.species])
        check(_lib.load().sgpr_set_mean(self._h, ptr(self._table(self.mean, 0.0)), ptr(vs)))

    def solve(self, K, Y, noise=0.01):
        """make_munu (gppotential.py:548-605 -> _regression :1204-1339, optimize=False) on the
        device: jitcholesky(M), choli = L^-1, mu = lstsq([K; sigma L^T], [Y; 0])."""
        K = f64(K).reshape(-1, self.m)
        Y = f64(Y).reshape(-1)
        mu = np.zeros(self.m)
        ridge, sigma = C.c_double(0), C.c_double(0)
        code = _lib.load().sgpr_solve(self._h, len(K), ptr(K), ptr(Y), float(noise), ptr(mu), None,
                                      C.addressof(ridge), C.addressof(sigma))
        if code == _lib.E_NOT_PD:
            raise RuntimeError("cholesky was not successful!")  # theforce/regression/algebra.py:45-46
        check(code)
        self.mu, self.ridge, self.sigma = mu, ridge.value, sigma.value
        self._choli, self._choli_on_device = None, True
        self.make_vscale()
        return mu

    def jitcholesky(self, A):
        """regression/algebra.py:29-47 on the device for any symmetric matrix: (L, ridge)."""
        A = f64(A)
        n = len(A)
        L = np.zeros((n, n))
        ridge = C.c_double(0)
        code = _lib.load().sgpr_jitcholesky(self._h, n, ptr(A), ptr(L), C.addressof(ridge))
        if code == _lib.E_NOT_PD:
            raise RuntimeError("cholesky was not successful!")
        check(code)
        return L, ridge.value

    def resolve(self, noise=0.01):
        """The same regression for another noise, re-using the factored [K | Y] of the last `solve`
        (the evaluations of _regression(optimize=True), gppotential.py:1265-1300)."""
        mu = np.zeros(self.m)
        ridge, sigma = C.c_double(0), C.c_double(0)
        # (choli = L^-1 and the ridge do not depend on the noise: they stay what the last solve returned)
        check(_lib.load().sgpr_resolve(self._h, float(noise), ptr(mu), None, C.addressof(ridge), C.addressof(sigma)))
        self.mu, self.ridge, self.sigma = mu, ridge.value, sigma.value
        return mu

    def resolve_many(self, noises):
        """mu for each of `noises` from the factored [K | Y] of the last solve, evaluated together on the device
        (the grid scan of the noise search); the installed weights do not change.  Returns [len(noises), m]."""
        noises = f64(noises).reshape(-1)
        out = np.zeros((len(noises), self.m))
        for a in range(0, len(noises), 64):
            part = np.zeros((min(64, len(noises) - a), self.m))
            check(_lib.load().sgpr_resolve_batch(self._h, len(part), ptr(f64(noises[a:a + 64])), ptr(part)))
            out[a:a + len(part)] = part
        return out

    def kernel_rows(self, numbers, positions, cell, pbc):
        """(Ke[m], Kf[3N,m], Kv[6,m]) of one data frame (gppotential.py:63-84, :495-497)."""
        numbers = i32(numbers)
        N = len(numbers)
        positions = f64(positions).reshape(N, 3)
        cell = f64(np.asarray(cell, float).reshape(3, 3))
        pbc = i32(np.asarray(pbc, bool).astype(np.int32))
        Ke, Kf, Kv = np.zeros(self.m), np.zeros((3 * N, self.m)), np.zeros((6, self.m))
        self.generation += 1
        check(_lib.load().sgpr_kernel_rows(self._h, N, ptr(numbers), ptr(positions), ptr(cell), ptr(pbc), ptr(Ke),
                                           ptr(Kf), ptr(Kv)))
        return Ke, Kf, Kv

    def kernel_columns(self, numbers, positions, cell, pbc, q_first, q_count):
        """The same rows restricted to inducing columns [q_first, q_first+q_count): the bordering
        step of add_inducing (gppotential.py:745-763)."""
        numbers = i32(numbers)
        N = len(numbers)
        positions = f64(positions).reshape(N, 3)
        cell = f64(np.asarray(cell, float).reshape(3, 3))
        pbc = i32(np.asarray(pbc, bool).astype(np.int32))
        Ke, Kf, Kv = np.zeros(q_count), np.zeros((3 * N, q_count)), np.zeros((6, q_count))
        self.generation += 1
        check(_lib.load().sgpr_kernel_columns(self._h, N, ptr(numbers), ptr(positions), ptr(cell), ptr(pbc),
                                              int(q_first), int(q_count), ptr(Ke), ptr(Kf), ptr(Kv)))
        return Ke, Kf, Kv

    # ------------------------------------------------------------------ resident training set
    def data_push(self, numbers, positions, cell, pbc, nv=6):
        """Append a data frame to the device-resident design matrix (PosteriorPotential.add_data,
        gppotential.py:730-743): its K_e / K_f / K_v rows are computed on the device and stay there."""
        numbers = i32(numbers)
        N = len(numbers)
        positions = f64(positions).reshape(N, 3)
        cell = f64(np.asarray(cell, float).reshape(3, 3))
        pbc = i32(np.asarray(pbc, bool).astype(np.int32))
        self.generation += 1
        check(_lib.load().sgpr_data_push(self._h, N, ptr(numbers), ptr(positions), ptr(cell), ptr(pbc), int(nv)))

    def data_pop(self, index=-1):
        """pop_1data (index -1) / popfirst_1data (index 0), gppotential.py:793-813."""
        check(_lib.load().sgpr_data_pop(self._h, int(index)))

    def data_clear(self):
        check(_lib.load().sgpr_data_clear(self._h))

    def data_info(self):
        n, rows = C.c_int32(0), C.c_int64(0)
        check(_lib.load().sgpr_data_info(self._h, C.addressof(n), C.addressof(rows)))
        return n.value, rows.value

    def data_matvec(self, v):
        """K v over all stored rows (frame-major: e, 3N f, nv v per frame)."""
        v = f64(v).reshape(self.m)
        out = np.zeros(self.data_info()[1])
        check(_lib.load().sgpr_data_matvec(self._h, ptr(v), ptr(out)))
        return out

    def data_fit_stats(self, v, Y):
        """(e_pred[frames], stats[7]) of K v against the targets Y, reduced on the device: the energy rows of K v and
        {sum d, sum |d|, sum d^2, sum y, sum y^2, max |y|, count} of d = K v - Y over the force / virial rows."""
        v = f64(v).reshape(self.m)
        Y = f64(Y).reshape(-1)
        n, rows = self.data_info()
        if len(Y) != rows:
            raise ValueError(f"data_fit_stats: {len(Y)} targets for {rows} stored rows")
        e, st = np.zeros(n), np.zeros(8)
        check(_lib.load().sgpr_data_fit_stats(self._h, ptr(v), ptr(Y), ptr(e), ptr(st)))
        return e, st[:7]

    def data_force_mae(self, V, Y):
        """mean |K_f v - Y_f| over the force rows for every row v of V [count, m] (sgpr_data_force_mae): the objective of
        the noise search, reduced on the device."""
        V = f64(V).reshape(-1, self.m)
        Y = f64(Y).reshape(-1)
        if len(Y) != self.data_info()[1]:
            raise ValueError(f"data_force_mae: {len(Y)} targets for {self.data_info()[1]} stored rows")
        out = np.zeros(len(V))
        check(_lib.load().sgpr_data_force_mae(self._h, len(V), ptr(V), ptr(Y), ptr(out)))
        return out

    def data_get(self):
        """The resident design matrix [rows, m] (diagnostics / tests)."""
        out = np.zeros((self.data_info()[1], self.m))
        if out.size:
            check(_lib.load().sgpr_data_get(self._h, ptr(out)))
        return out

    def data_factor(self, Y, with_energies=True):
        """The first stage of data_solve alone: [R1, z] of the resident [K | Y] for resolve / resolve_many."""
        Y = f64(Y).reshape(-1)
        if len(Y) != self.data_info()[1]:
            raise ValueError(f"data_factor: {len(Y)} targets for {self.data_info()[1]} stored rows")
        self.generation += 1
        code = _lib.load().sgpr_data_factor(self._h, ptr(Y), int(bool(with_energies)))
        if code == _lib.E_NOT_PD:
            raise RuntimeError("cholesky was not successful!")
        check(code)

    def data_solve(self, Y, with_energies=True, noise=0.01):
        """`solve` on the resident matrix (Y in its row order)."""
        Y = f64(Y).reshape(-1)
        if len(Y) != self.data_info()[1]:
            raise ValueError(f"data_solve: {len(Y)} targets for {self.data_info()[1]} stored rows")
        mu = np.zeros(self.m)
        ridge, sigma = C.c_double(0), C.c_double(0)
        self.generation += 1
        code = _lib.load().sgpr_data_solve(self._h, ptr(Y), int(bool(with_energies)), float(noise), ptr(mu), None,
                                           C.addressof(ridge), C.addressof(sigma))
        if code == _lib.E_NOT_PD:
            raise RuntimeError("cholesky was not successful!")  # theforce/regression/algebra.py:45-46
        check(code)
        self.mu, self.ridge, self.sigma = mu, ridge.value, sigma.value
        self._choli, self._choli_on_device = None, True
        self.make_vscale()
        return mu

    def fit(self, frames, noise=0.01):
        """set_data + make_munu (gppotential.py:484-509, :548-605) for a list of labelled frames
        dict(numbers, positions, cell, pbc, energy, forces[, stress]): builds K = [Ke; Kf; Kv] and
        Y = [E - mean; F; V * stress] and solves for mu on the device.  Frames without `stress`
        contribute no virial rows."""
        Ke, Kf, Kv, Ye, Yf, Yv = [], [], [], [], [], []
        for fr in frames:
            ke, kf, kv = self.kernel_rows(fr["numbers"], fr["positions"], fr["cell"], fr["pbc"])
            Ke.append(ke[None]); Kf.append(kf)
            mean = sum(self.mean.get(int(z), 0.0) for z in fr["numbers"])
            Ye.append([fr["energy"] - mean]); Yf.append(np.asarray(fr["forces"], float).reshape(-1))
            if fr.get("stress") is not None:
                vol = abs(np.linalg.det(np.asarray(fr["cell"], float).reshape(3, 3)))
                Kv.append(kv); Yv.append(np.asarray(fr["stress"], float) * vol)
        K = np.concatenate(Ke + Kf + Kv)
        Y = np.concatenate([np.concatenate(Ye)] + Yf + Yv)
        return self.solve(K, Y, noise=noise)

    def make_vscale(self):
        out = np.zeros(len(self.species))
        check(_lib.load().sgpr_make_vscale(self._h, ptr(out)))
        self._vscale = {z: float(v) for z, v in zip(self.species, out) if np.isfinite(v)}
        return self._vscale

    # ------------------------------------------------------------------ prediction
    def predict(self, numbers, positions, cell, pbc, rank=0, world=1, cov=False, beta=True):
        """One pass of the hot path (calculator/active.py:425-502): returns a dict with energy,
        forces [N,3], stress [6], and optionally beta [N] (covloss) and cov [N,m]."""
        numbers = i32(numbers)
        N = len(numbers)
        positions = f64(positions).reshape(N, 3)
        cell = f64(np.asarray(cell, float).reshape(3, 3))
        pbc = i32(np.asarray(pbc, bool).astype(np.int32))
        E = C.c_double(0)
        F = np.empty((N, 3))  # every output is written by the call (a failure raises)
        stress = np.zeros(6)
        b = np.empty(N) if beta else None
        K = np.zeros((N, self.m)) if cov else None
        self.generation += 1
        check(_lib.load().sgpr_compute(self._h, N, ptr(numbers), ptr(positions), ptr(cell), ptr(pbc), rank, world,
                                       C.addressof(E), ptr(F), ptr(stress), ptr(b), ptr(K)))
        return dict(energy=E.value, forces=F, stress=stress, beta=b, cov=K)

    def predict_view(self, numbers, positions, cell, pbc, rank=0, world=1):
        """predict() for callers in a loop (ActiveCalculator.calculate): the same pass, but forces / beta / stress come
        back as numpy VIEWS of the page-locked buffer the device wrote them to (include/sgpr_hip.h: sgpr_compute_view) — valid
        until the call after next —, and what does not change between calls (the int32 numbers, pbc, the views themselves)
        is kept instead of being rebuilt: ~20 us less per call at 4096 atoms."""
        N = len(numbers)
        if N == 0:   # an empty frame: zeros, as predict() gives (sgpr_compute_view has no buffer to hand out)
            return self.predict(numbers, positions, cell, pbc, rank=rank, world=world)
        c = self._pv
        if c is None or c["N"] != N or c["src"] is not numbers:
            n32 = i32(numbers)
            if c is not None and c["N"] == N and np.array_equal(c["n32"], n32):
                c["src"] = numbers
            else:
                c = self._pv = dict(N=N, src=numbers, n32=n32, n32p=ptr(n32), views={}, out=C.c_void_p(0))
                c["outp"] = C.addressof(c["out"])
        if positions.dtype != np.float64 or not positions.flags.c_contiguous:
            positions = f64(positions)
        if cell.dtype != np.float64 or not cell.flags.c_contiguous:
            cell = f64(cell)
        pb = (bool(pbc[0]), bool(pbc[1]), bool(pbc[2]))
        if c.get("pb") != pb:
            c["pb"], c["pbc32"] = pb, i32(np.asarray(pb, np.int32))
            c["pbcp"] = ptr(c["pbc32"])
        self.generation += 1
        code = _lib.load().sgpr_compute_view(self._h, N, c["n32p"], positions.ctypes.data, cell.ctypes.data, c["pbcp"], rank, world,
                                             c["outp"])
        if code:
            check(code)
        addr = c["out"].value
        v = c["views"].get(addr)
        if v is None:
            buf = np.frombuffer((C.c_double * (4 * N + 17)).from_address(addr), dtype=np.float64)
            v = c["views"][addr] = (buf[:3 * N].reshape(N, 3), buf[3 * N:4 * N], buf[4 * N:4 * N + 1].reshape(()), buf[4 * N + 11:4 * N + 17])
        return dict(energy=v[2], forces=v[0], stress=v[3], beta=v[1], cov=None)

    # ------------------------------------------------------------------ device-resident molecular dynamics
    MD_SCALARS = 16  # per evaluation: E, virial[9], overflow word, largest covloss, sum m v^2, 3 spare

    def md_begin(self, numbers, positions, cell, pbc, masses, velocities=None, dt=1.0, friction=0.0, kT=0.0, seed=0, ttime=None,
                 pfactor=None, externalstress=0.0, mask=None, iso=False, fixed=None, ml_filter=None, filter_init=None):
        """State of an MD run into device memory (cl/md.py:117-128 drives ase.md.langevin around calculate();
        here the integrator is part of the step's last kernel).  dt, friction and kT in the caller's units
        (workloads.FS / ase_shim.kB for fs / K).
          pfactor (with ttime): a barostat, the moving cell of ase.md.npt.NPT (sgpr_md_barostat); md_committee(members,
        moving_cell=True) may follow: the committee then runs in the moving cell.
          fixed: held atoms ([N] booleans: ase.constraints.FixAtoms) or Cartesian components ([N, 3]: FixCartesian), True =
        held (sgpr_md_fix; None or nothing held: the run without a mask).  The integrator sees F = 0 on a held component — the
        forces md_state reports stay the model's —, its velocity is exactly 0 from here on (the caller's value is dropped), it
        draws no noise and keeps the coordinate it was uploaded with, bit for bit.  Nose-Hoover then works on the
        g = 3N - n_fixed remaining degrees of freedom: tfact = 2 / (g kT ttime^2), K0 = g kT / 2 (the project's own definition:
        ase.md.npt.NPT takes no constraints), and temperatures are sum m v^2 / (g kB) (md_dof()).  Not with a barostat.
          ml_filter: the shrink factor (0 < s < 1) of the filter of model-update jumps (sgpr_md_filter; the reference's
        FilterDeltas, cl/md.py:76-79): per configuration A <- (A + pushed jumps) s, and the integrator sees
        F - clip(A_f, -1, 1) and, with a barostat, stress - A_s; what md_state and the rows report stays the model's.
        filter_init: (f [N, 3], s [6]) the accumulators of configuration 0 (either None: zeros).  md_filter_push adds the jumps
        of an update between two md_run calls, md_filter_state returns the accumulators.  None: the run without a filter."""
        from .workloads import fixed_mask
        numbers = i32(numbers)
        N = len(numbers)
        fx = fixed_mask(fixed, N)
        self._md = dict(N=N, numbers=numbers, cell=f64(np.asarray(cell, float).reshape(3, 3)), masses=f64(masses), hdt=0.5 * dt, fixed=fx)
        if pfactor is not None:
            if fx is not None:
                raise NotImplementedError("md_begin: held components (fixed) with a barostat (pfactor): the moving-cell dynamics "
                                          "run without a mask")
            if ttime is None:
                raise ValueError("a barostat (pfactor) needs the Nose-Hoover thermostat (ttime)")
            from .npt import zero_mean_momentum   # (NPT.__init__ removes the mean momentum: the host twin starts from the same bits)
            velocities = zero_mean_momentum(np.zeros((N, 3)) if velocities is None else velocities, masses)
        v = None if velocities is None else f64(velocities).reshape(N, 3)
        self.generation += 1
        check(_lib.load().sgpr_md_begin(self._h, N, ptr(numbers), ptr(f64(positions).reshape(N, 3)), ptr(self._md["cell"]),
                                        ptr(i32(np.asarray(pbc, bool).astype(np.int32))), ptr(self._md["masses"]), ptr(v),
                                        float(dt), float(friction), float(kT)))
        # seed != 0: md_run(noise=None) draws the Langevin deviates on the device (counter-based, md_deviates returns them)
        check(_lib.load().sgpr_md_seed(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF))
        self._md_fix(fx)
        # ttime: Nose-Hoover NVT with that time constant instead of the Langevin / velocity-Verlet step (the reference's
        # default dynamics, cl/md.py:131-166: ase.md.npt.NPT with pfactor = None)
        if ttime is not None:
            check(_lib.load().sgpr_md_thermostat(self._h, 1, float(ttime), float(kT)))
            self._md["nh"] = True
        # pfactor: ... and a barostat — the moving cell of cl/md.py:131-166 (ase.md.npt.NPT with a pfactor; npt.py restates it,
        # workloads.npt_moving_cell is the host twin).  externalstress: a pressure or six Voigt components; mask: 3 or 3 x 3;
        # iso: the trace of the strain rate only (set_fraction_traceless(0)).  The cell must be upper triangular.
        if pfactor is not None:
            ext = np.asarray(externalstress, float)
            ext = np.array([-float(ext)] * 3 + [0.0] * 3) if ext.ndim == 0 else f64(ext).reshape(6)
            mk = np.not_equal(np.ones(3) if mask is None else np.asarray(mask), 0)
            mk = f64((np.outer(mk, mk) if mk.shape == (3,) else mk.reshape(3, 3)).astype(float))
            check(_lib.load().sgpr_md_barostat(self._h, float(pfactor), ptr(f64(ext)), ptr(mk), 0.0 if iso else 1.0))
            self._md["npt"] = True
        if ml_filter is not None:
            f0, s0 = (None, None) if filter_init is None else filter_init
            f0 = None if f0 is None else f64(np.asarray(f0, float)).reshape(N, 3)
            s0 = None if s0 is None else f64(np.asarray(s0, float)).reshape(6)
            check(_lib.load().sgpr_md_filter(self._h, float(ml_filter), ptr(f0), ptr(s0)))
            self._md["shrink"] = float(ml_filter)
        self._md["t"] = 0

    def md_filter_push(self, dforces, dstress=None):
        """The jump of a model update — calculate()'s `deltas` after a halt — into the filter's accumulators of the current
        configuration (sgpr_md_filter_push), between two md_run calls: dforces [N, 3] (or None), dstress [6] (or None; ignored at
        constant cell).  The repeated evaluation shrinks the sum and applies it."""
        N = self._md["N"]
        dF = None if dforces is None else f64(np.asarray(dforces, float)).reshape(N, 3)
        dS = None if dstress is None else f64(np.asarray(dstress, float)).reshape(6)
        check(_lib.load().sgpr_md_filter_push(self._h, ptr(dF), ptr(dS)))

    def md_filter_state(self):
        """(f [N, 3], s [6]): the filter's accumulators of the current configuration — what its evaluation will shrink and
        apply, and what md_begin(filter_init=) takes to go on from here (sgpr_md_filter_state)."""
        f, s_ = np.empty((self._md["N"], 3)), np.empty(6)
        check(_lib.load().sgpr_md_filter_state(self._h, ptr(f), ptr(s_)))
        return f, s_

    META_KINDS = {"distance": 0, "posvar": 1, "qlvar": 2}

    def md_meta(self, cvs, sigma, w, tem=None, pace=1, hills=None, capacity=None, merge=None):
        """Metadynamics for the run begun by md_begin (sgpr_md_meta; md_meta.inc has the scheme, workloads.meta_bias is the host
        twin and the definition; the reference's calculator/meta.py): from the next md_run on every configuration is evaluated
        with the bias V = w kde(cv) — tem (K): the well-tempered log(1 + w kde gamma) / gamma, gamma = 1 / (kB tem) — of the
        hills deposited by the configurations before it, and configuration n deposits its own when n % pace == 0.  Energy,
        forces and stress of the rows, md_state and the frame record include the bias; the covloss gate does not see it.
          cvs: the components of the collective variable in the order they are concatenated, ("distance", i, j) = |x_j - x_i|
        and ("posvar", index, select) = x_index - (1/n) sum of the other atoms of species `select` (None: all atoms; n counts
        the index atom where it is among them) — raw coordinates, no minimum image —, and ("qlvar", index, j, cutoff, l) = the
        Steinhardt bond-order parameters Q_l, one dimension per entry of l (0 ... 12), of atom `index` over its neighbours of
        species j with r < cutoff <= the model's cutoff, from the step's own neighbour list (sgpr_md_meta_ql; kind 2 of
        md_meta.inc; workloads.ql_dim) — at most 4 components and 6 dimensions.
        sigma: a scalar or [D].  hills: [H, D] CV values (or (cv [H, D], V [H])) that stand from the start — a restart, or
        md_meta_hills() of this run when it needs more room; capacity: rows of hills (default: those given + 4096) — md_run
        refuses a call that would pass it before it enqueues anything, md_meta again with the rows of md_meta_hills(count=
        md_meta_info()["below"]) and a larger capacity lets the run go on with the same bits.  cvs = None or (): no bias.
        Langevin, velocity Verlet and Nose-Hoover at constant cell on one rank, with or without fixed=, ml_filter= and
        md_record; a barostat, a relaxation, a band, a committee and several ranks: NotImplementedError (the host loop
        around calculate() serves them).
          merge = CH: the merged form (sgpr_md_meta_merge; workloads.meta_density(merge=) is the definition) — the hills are
        merged by bin, chunk after chunk of CH rows, inside the loop, and the cost of the bias grows with the bins visited, not
        with time; md_meta_table() fetches the table.  None: every hill on its own, today's launches and bits."""
        lib = _lib.load()
        if not cvs:
            check(lib.sgpr_md_meta(self._h, 0, None, None, 0.0, 0.0, 1, 1, 0, None, None))
            self._md.pop("meta_D", None)
            return
        if merge is not None and int(merge) < 1:
            raise ValueError(f"md_meta: merge is a chunk length >= 1 or None, not {merge}")
        from .ase_shim import kB
        spec, D = [], 0
        for q, c in enumerate(cvs):
            kind = self.META_KINDS[c[0]]
            if kind == 2:
                # (the parameters of a qlvar are staged for the attach below)
                if c[1] is None:
                    raise ValueError("md_meta: a qlvar names its atom (Meta.resolve(numbers) fixes a Qlvar(index=None))")
                ls = i32(np.asarray([int(l) for l in c[4]], np.int32))
                check(lib.sgpr_md_meta_ql(self._h, q, float(c[3]), len(ls), ptr(ls)))
                spec.append((2, int(c[1]), int(c[2])))
                D += len(ls)
                continue
            spec.append((kind, int(c[1]), int(c[2]) if kind == 0 else (-1 if c[2] is None else int(c[2]))))
            D += 1 if kind == 0 else 3
        sg = f64(np.broadcast_to(np.asarray(sigma, float).reshape(-1), (D,)) if np.size(sigma) == 1 else np.asarray(sigma, float).reshape(-1))
        if len(sg) != D:
            raise ValueError(f"md_meta: sigma is a scalar or one value per dimension ({D}), not {len(sg)}")
        hv = None
        if isinstance(hills, tuple):
            hills, hv = hills
        hc = np.zeros((0, D)) if hills is None else f64(np.asarray(hills, float)).reshape(-1, D)
        hv = None if hv is None else f64(np.asarray(hv, float)).reshape(len(hc))
        cap = len(hc) + 4096 if capacity is None else int(capacity)
        _attach(lib.sgpr_md_meta(self._h, len(spec), ptr(i32(np.asarray(spec, np.int32).reshape(-1))), ptr(sg), float(w),
                                 0.0 if tem is None else float(kB * tem), int(pace), cap, len(hc), ptr(hc) if len(hc) else None, ptr(hv)))
        self._md["meta_D"] = D
        if merge is not None:
            check(lib.sgpr_md_meta_merge(self._h, int(merge)))

    def md_meta_table(self):
        """(centres [T, D], counts [T], rows_merged) of the merged bias (sgpr_md_meta_table; md_meta(merge=)): one entry per
        occupied bin in the order of the first hill that fell into it, as the current configuration sees it — the reference's
        Gaussian_kde.histogram() — and the number of hill rows it was merged from."""
        lib = _lib.load()
        n, rows = C.c_int64(0), C.c_int64(0)
        check(lib.sgpr_md_meta_table(self._h, None, None, C.addressof(n), C.addressof(rows)))
        centres, counts = np.zeros((n.value, self._md["meta_D"])), np.zeros(n.value)
        if n.value:
            check(lib.sgpr_md_meta_table(self._h, ptr(centres), ptr(counts), C.addressof(n), C.addressof(rows)))
        return centres, counts, rows.value

    def md_meta_info(self):
        """dict(D, below, held, capacity) of the run's bias (sgpr_md_meta_info): below = the hills below the current
        configuration (what md_meta(hills=) takes to go on from here), held = those and the current configuration's own row
        after a halted or `final` md_run (what md_meta_hills serves)."""
        D = C.c_int(0)
        below, held, cap = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(_lib.load().sgpr_md_meta_info(self._h, C.addressof(D), C.addressof(below), C.addressof(held), C.addressof(cap)))
        return dict(D=D.value, below=below.value, held=held.value, capacity=cap.value)

    def md_meta_hills(self, first=0, count=None):
        """(cv [count, D], V [count]): rows first ... first + count - 1 of the hills that stand (default: all from `first`) — where
        each was deposited and the bias its configuration saw (sgpr_md_meta_hills)."""
        info = self.md_meta_info()
        count = info["held"] - int(first) if count is None else int(count)
        cv, V = np.zeros((max(count, 0), info["D"])), np.zeros(max(count, 0))
        if count > 0:
            check(_lib.load().sgpr_md_meta_hills(self._h, int(first), count, ptr(cv), ptr(V)))
        return cv, V

    def _md_fix(self, fx):
        """The held components of the run just begun (sgpr_md_fix: before the thermostat / the relaxation is set)."""
        if fx is not None:
            check(_lib.load().sgpr_md_fix(self._h, ptr(np.ascontiguousarray(fx, dtype=np.uint8))))

    def md_dof(self):
        """Degrees of freedom of the run: 3N less the held components."""
        fx = self._md.get("fixed")
        return 3 * self._md["N"] - (0 if fx is None else int(fx.sum()))

    def relax_begin(self, numbers, positions, cell, pbc, fmax, cell_relax=False, mask=None, fixed=None, optimizer="FIRE", **fire):
        """State of a FIRE relaxation into device memory (sgpr_md_relax: ase/optimize/fire.py on the positions and, with
        cell_relax, on the cell through ase.constraints.UnitCellFilter(atoms, mask=mask)'s coordinates; workloads.fire_relax is
        the host twin).  fire: dt, maxstep, dtmax, nmin, finc, fdec, astart, fa (ASE's defaults).  md_run / md_state / md_cells /
        md_end then serve the relaxation as they serve an MD run: md_run's halt code 3 = converged at its last row, nothing
        moved; its rows carry max |G_row|^2, G.v, dt and a in the columns 12..15; md_cells returns (cells, D).
          fixed: held atoms ([N]) or components ([N, 3]), True = held (sgpr_md_fix): the optimizer sees F = 0 there, the entries
        of G are zero in FIRE's sums and in max |G_row|^2 — convergence is judged on the free components, the forces reported
        stay the model's —, and the coordinate stays: x itself at constant cell, bit for bit; with cell_relax the undeformed
        r, x = r D^T following the cell (FixAtoms inside UnitCellFilter).
          optimizer = "LBFGS": L-BFGS without line search in the place of FIRE (sgpr_md_relax_lbfgs, md_lbfgs.inc;
        workloads.lbfgs_relax is the host twin), with ASE's keywords memory (1 ... 128), maxstep, alpha, damping in the place
        of FIRE's; the columns 12..15 are then max |G_row|^2, p.G, the scale applied to the step and the valid pairs in use,
        and relax_reset empties the history."""
        from .workloads import FIRE_DEFAULTS, LBFGS_DEFAULTS, fixed_mask
        if optimizer not in ("FIRE", "LBFGS"):
            raise ValueError(f"relax_begin: optimizer = 'FIRE' or 'LBFGS', not {optimizer!r}")
        lbfgs = None
        if optimizer == "LBFGS":
            unknown = set(fire) - set(LBFGS_DEFAULTS)
            if unknown:
                raise TypeError(f"relax_begin: unknown L-BFGS keywords {sorted(unknown)}")
            lbfgs, fire = dict(LBFGS_DEFAULTS, **fire), {}
        unknown = set(fire) - set(FIRE_DEFAULTS)
        if unknown:
            raise TypeError(f"relax_begin: unknown FIRE keywords {sorted(unknown)}")
        numbers = i32(numbers)
        N = len(numbers)
        fx = fixed_mask(fixed, N)
        self._md = dict(N=N, numbers=numbers, cell=f64(np.asarray(cell, float).reshape(3, 3)), masses=np.ones(N), hdt=0.0, relax=True, npt=True,
                        fixed=fx)
        self.generation += 1
        lib = _lib.load()
        check(lib.sgpr_md_begin(self._h, N, ptr(numbers), ptr(f64(positions).reshape(N, 3)), ptr(self._md["cell"]),
                                ptr(i32(np.asarray(pbc, bool).astype(np.int32))), None, None, 1.0, 0.0, 0.0))
        par = dict(FIRE_DEFAULTS)
        par.update(fire)
        fp = f64([par[k] for k in ("dt", "maxstep", "dtmax", "nmin", "finc", "fdec", "astart", "fa")])
        mk = None if mask is None else f64(np.asarray(mask, float).reshape(6))
        self._md_fix(fx)
        check(lib.sgpr_md_relax(self._h, float(fmax), ptr(fp), int(bool(cell_relax)), ptr(mk)))
        if lbfgs is not None:
            check(lib.sgpr_md_relax_lbfgs(self._h, int(lbfgs["memory"]), float(lbfgs["maxstep"]), float(lbfgs["alpha"]), float(lbfgs["damping"])))
        self._md["t"] = 0

    def relax_reset(self):
        """optimizer.initialize() of the relaxation on the device: v = 0; dt, a, nsteps back to their start (FIRE); the history
        emptied (L-BFGS)."""
        check(_lib.load().sgpr_md_relax_reset(self._h))

    def neb_begin(self, numbers, images, cell, pbc, fmax, k=0.1, climb=False, fixed=None, **fire):
        """A nudged elastic band under FIRE into device memory (sgpr_md_neb: ASE's default `aseneb` method, md_neb.inc;
        workloads.neb_fire is the host twin and the definition).  images [K + 2, N, 3]: images 0 and K + 1 are the ends, never
        evaluated or moved; the K <= 16 interior ones share numbers, cell (constant) and pbc and are evaluated by this one
        model, one plain step each per evaluation of the band.  k: the spring constant; climb: the image of highest energy
        climbs; fixed: held atoms ([N]) or components ([N, 3]) of every image; fire: FIRE's keywords (ASE's defaults).
        md_run then serves the band — (scalars, halt code): rows carry E of the highest image, its index and the index of the
        image with the largest covloss (1 ... K) in columns 0..2, overflow, largest covloss, max |G_row|^2, G.v, dt and a in
        10..15; code 1 = the covloss gate (nothing moved), 3 = converged —; neb_state returns the images, neb_info the
        energies and largest covlosses per image of the last call's evaluations, neb_reset re-initialises the optimizer.
          The displacement of an atom between neighbouring images must stay well inside half a cell (workloads.neb_check_band:
        refused at the start, the caller's to keep for the rest of the run).  One rank; no thermostat, committee, filter or
        frame record."""
        from .workloads import FIRE_DEFAULTS, fixed_mask
        unknown = set(fire) - set(FIRE_DEFAULTS)
        if unknown:
            raise TypeError(f"neb_begin: unknown FIRE keywords {sorted(unknown)}")
        numbers = i32(numbers)
        N = len(numbers)
        R = f64(np.asarray(images, float))
        if R.ndim != 3 or R.shape[1:] != (N, 3) or len(R) < 2:
            raise ValueError(f"neb_begin: images is [K + 2, N, 3] for N = {N} atoms, not {R.shape}")
        K = len(R) - 2
        fx = fixed_mask(fixed, N)
        md = dict(N=N, numbers=numbers, cell=f64(np.asarray(cell, float).reshape(3, 3)), masses=np.ones(N), hdt=0.0, neb=K, fixed=fx)
        self._md = None   # (no run until sgpr_md_neb has accepted the band)
        self.generation += 1
        lib = _lib.load()
        check(lib.sgpr_md_begin(self._h, N, ptr(numbers), ptr(f64(R[min(1, len(R) - 1)])), ptr(md["cell"]),
                                ptr(i32(np.asarray(pbc, bool).astype(np.int32))), None, None, 1.0, 0.0, 0.0))
        par = dict(FIRE_DEFAULTS)
        par.update(fire)
        fp = f64([par[q] for q in ("dt", "maxstep", "dtmax", "nmin", "finc", "fdec", "astart", "fa")])
        try:
            self._md_fix(fx)
            check(lib.sgpr_md_neb(self._h, K, ptr(R), float(fmax), float(k), int(bool(climb)), ptr(fp)))
        except Exception:
            lib.sgpr_md_end(self._h)   # (a refused band leaves no half-begun run behind: _md stays None and md_run says so)
            raise
        md["t"] = 0
        self._md = md

    def neb_reset(self):
        """optimizer.initialize() of the band on the device: v = 0; dt, a, nsteps back to their start."""
        check(_lib.load().sgpr_md_neb_reset(self._h))

    def _replicas(self, who, key, noun):
        """R of the run whose configuration is R replicas under `key` ("neb": a band's interior images, "pimd": a polymer's beads)."""
        if not (getattr(self, "_md", None) and self._md.get(key)):
            raise RuntimeError(f"{who}: no {noun} on this model: {key}_begin first (a refused {key}_begin leaves none)")
        return self._md[key]

    def _replica_state(self, key, noun, which, results, vname, **more):
        """What neb_state and pimd_state share: positions [R, N, 3], the mode's velocity under `vname`, what the mode adds
        (`more`), and with results=True forces [R, N, 3], beta [R, N], energy [R], stress [R, 6] off the replicas' packed results."""
        R = self._replicas(f"{key}_state", key, noun)
        N = self._md["N"]
        x, v = np.empty((R, N, 3)), np.empty((R, N, 3))
        packed = np.empty((R, 4 * N + 11)) if results else None
        check(getattr(_lib.load(), f"sgpr_md_{key}_state")(self._h, ptr(x), ptr(v), ptr(packed), int(which)))
        out = {"positions": x, vname: v, **more}
        if results:
            stress = np.zeros((R, 6))
            for i in range(R):
                check(_lib.load().sgpr_stress_from_virial(ptr(f64(packed[i, 4 * N + 1:4 * N + 10])), ptr(self._md["cell"]), ptr(stress[i])))
            out.update(forces=packed[:, :3 * N].reshape(R, N, 3).copy(), beta=packed[:, 3 * N:4 * N].copy(), energy=packed[:, 4 * N].copy(),
                       stress=stress)
        return out

    def _replica_info(self, key, noun, half):
        """(E [done, R], covmax [done, R]) off the rows E[half] | covmax[half] of the last md_run that stand."""
        R = self._replicas(f"{key}_info", key, noun)
        done = self._md.get("rep_done", 0)
        out = np.zeros((done, 2 * half))
        if done:
            check(getattr(_lib.load(), f"sgpr_md_{key}_info")(self._h, 0, done, ptr(out)))
        return out[:, :R].copy(), out[:, half:half + R].copy()

    def neb_state(self, which=0, results=False):
        """The K interior images of the current band (which = -1: the one evaluated before it): dict(positions [K, N, 3],
        velocities [K, N, 3] FIRE's); with results=True — where the last md_run evaluated that band: which = 0 after a halted or
        `final` call, -1 after one that ran through — also forces [K, N, 3], beta [K, N], energy [K], stress [K, 6]."""
        return self._replica_state("neb", "band", which, results, "velocities")

    def neb_info(self):
        """(E [done, K], covmax [done, K]): energy and largest covloss of every interior image at the evaluations of the last
        md_run that stand (sgpr_md_neb_info)."""
        return self._replica_info("neb", "band", 16)

    PIMD_MAX = 32   # beads of a polymer (md_pimd.inc)

    def pimd_begin(self, numbers, beads, cell, pbc, masses, velocities=None, dt=1.0, kT=0.0, friction=1e-3, pile_lambda=1.0, seed=0):
        """A ring polymer of P beads into device memory (sgpr_md_pimd: path-integral MD under BAOAB with the PILE-L thermostat,
        md_pimd.inc; workloads.pimd_baoab is the host twin and the definition).  beads [P, N, 3], velocities [P, N, 3] (None:
        zeros): the P <= 32 beads share numbers, cell (constant), pbc and masses and are evaluated by this one model, one plain
        step each per evaluation of the polymer.  kT: the physical one (the polymer is sampled at P kT); dt, kT, friction in the
        units of workloads.FS / ase_shim.kB, as md_begin takes them; friction: the centroid's, pile_lambda: gamma_k =
        2 pile_lambda w_k of the other modes (friction = 0 with 1/2: TRPMD, with 0: microcanonical RPMD).  seed != 0:
        md_run(noise=None) draws the deviates on the device — those md_deviates returns for t = n P + k.
          md_run then serves the polymer — noise [nevals, P, N, 3] (mode k, caller atom order); rows carry the mean energy of
        the beads in column 0, the bead (1 ... P) with the largest covloss in 1, overflow, largest covloss, sum m v^2 over all
        beads (closed | before the closing half kick) in 10..13, the centroid-virial kinetic energy in 14, the spring energy in
        15; code 1 = the covloss gate (nothing moved) —; pimd_state returns the beads, pimd_info the energies and largest
        covlosses per bead of the last call's evaluations.  One rank, constant cell; no other thermostat, committee, bias,
        filter, mask or frame record."""
        numbers = i32(numbers)
        N = len(numbers)
        R = f64(np.asarray(beads, float))
        if R.ndim != 3 or R.shape[1:] != (N, 3):
            raise ValueError(f"pimd_begin: beads is [P, N, 3] for N = {N} atoms, not {R.shape}")
        P = len(R)
        if P < 1:
            raise ValueError("pimd_begin: a polymer has at least one bead")
        v = None if velocities is None else f64(np.asarray(velocities, float)).reshape(P, N, 3)
        md = dict(N=N, numbers=numbers, cell=f64(np.asarray(cell, float).reshape(3, 3)), masses=f64(masses), hdt=0.5 * dt, pimd=P, fixed=None)
        self._md = None   # (no run until sgpr_md_pimd has accepted the polymer)
        self.generation += 1
        lib = _lib.load()
        check(lib.sgpr_md_begin(self._h, N, ptr(numbers), ptr(f64(R[0])), ptr(md["cell"]), ptr(i32(np.asarray(pbc, bool).astype(np.int32))),
                                ptr(md["masses"]), None, float(dt), float(friction), float(kT)))
        try:
            check(lib.sgpr_md_seed(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF))
            check(lib.sgpr_md_pimd(self._h, P, ptr(R), ptr(v), float(kT), float(friction), float(pile_lambda)))
        except Exception:
            lib.sgpr_md_end(self._h)   # (a refused polymer leaves no half-begun run behind: _md stays None and md_run says so)
            raise
        md["t"] = 0
        self._md = md

    def pimd_state(self, which=0, results=False):
        """The P beads of the current configuration (which = -1: the one evaluated before it): dict(positions [P, N, 3],
        velocities_pre [P, N, 3] before the closing half kick, pending: whether one is due); with results=True — where the last
        md_run evaluated that configuration: which = 0 after a halted or `final` call, -1 after one that ran through — also
        forces [P, N, 3], beta [P, N], energy [P], stress [P, 6] and velocities [P, N, 3], the closing half kick applied."""
        self._replicas("pimd_state", "pimd", "polymer")   # (no polymer: said before _md is read)
        pending = self._md["t"] + which > 0
        out = self._replica_state("pimd", "polymer", which, results, "velocities_pre", pending=pending)
        if results:
            v = out["velocities_pre"]
            out["velocities"] = v + self._md["hdt"] * out["forces"] / self._md["masses"][None, :, None] if pending else v.copy()
        return out

    def pimd_info(self):
        """(E [done, P], covmax [done, P]): energy and largest covloss of every bead at the evaluations of the last md_run that
        stand (sgpr_md_pimd_info)."""
        return self._replica_info("pimd", "polymer", 32)

    def md_deviates(self, t_first, count):
        out = np.empty((int(count), self._md["N"], 3))
        check(_lib.load().sgpr_md_deviates(self._h, int(t_first), int(count), ptr(out)))
        return out

    def md_run(self, nevals, noise=None, ediff=0.0, final=False):
        """Evaluate `nevals` configurations starting with the current one, integrating between them on the device
        (noise: [nevals, N, 3] standard normal deviates or None; a polymer, pimd_begin: [nevals, P, N, 3]).  Returns (scalars [done, 16], halt code): code 1 =
        the last row's largest covloss reached ediff and the state is that configuration (calculator/active.py:492-499),
        2 = a neighbour capacity overflowed at evaluation `done` (repeat the call), 3 (a relaxation, relax_begin) = the last
        row's configuration has converged and is the state."""
        if not getattr(self, "_md", None):
            raise RuntimeError("md_run: no run on this model: md_begin, relax_begin or neb_begin first (a refused begin leaves none)")
        N = self._md["N"]
        if noise is not None:
            noise = f64(noise).reshape((-1, self._md["pimd"], N, 3) if self._md.get("pimd") else (-1, N, 3))
            assert len(noise) >= nevals, "one row of noise per evaluation"
        sc = np.zeros((nevals, self.MD_SCALARS))
        done, code = C.c_int(0), C.c_int(0)
        self.generation += 1
        check(_lib.load().sgpr_md_run(self._h, int(nevals), ptr(noise), float(ediff), int(bool(final)), ptr(sc),
                                      C.addressof(done), C.addressof(code)))
        self._md["record_call"] = self._md.get("record")   # (what this call recorded: md_frames)
        self._md["rep_done"] = done.value   # (the rows of a band's or a polymer's record that stand: neb_info, pimd_info)
        if self._md.get("npt") or self._md.get("pimd"):   # (where the state is now: sgpr_md_run's rules)
            t0 = self._md["t"]
            self._md["run"] = (t0, done.value)
            self._md["t"] = t0 + (done.value - 1 if (code.value in (1, 3) or (code.value == 0 and final)) else done.value)
        return sc[:done.value], code.value

    def md_cells(self, first=None, count=None):
        """Moving-cell runs: (cells [count, 3, 3], eta [count, 3, 3]) of the configurations first ... first + count - 1 of the
        trajectory; default: those the last md_run evaluated.  The current configuration can always be asked for."""
        if first is None:
            first, count = self._md.get("run", (0, 0))
        count = 1 if count is None else int(count)
        out = np.zeros((count, 18))
        if count:
            check(_lib.load().sgpr_md_cells(self._h, int(first), count, ptr(out)))
        return out[:, :9].reshape(count, 3, 3).copy(), out[:, 9:].reshape(count, 3, 3).copy()

    def md_state(self, which=0, results=False):
        """Positions, velocities of the current configuration (which = -1: the one before it); with results=True also
        the forces / covloss / energy / stress of its last evaluation, and the velocities include the closing half kick
        of that evaluation (what an observer of the trajectory sees, workloads.langevin_nvt)."""
        N = self._md["N"]
        x, v = np.empty((N, 3)), np.empty((N, 3))
        pend = C.c_int(0)
        packed = np.empty(4 * N + 11) if results else None
        check(_lib.load().sgpr_md_state(self._h, ptr(x), ptr(v), C.addressof(pend), ptr(packed), int(which)))
        out = dict(positions=x, velocities_pre=v, pending=bool(pend.value))
        cell = self._md["cell"]
        if self._md.get("npt"):   # the cell these positions belong to, and its strain rate
            c, e = self.md_cells(self._md["t"] + which, 1)
            cell = out["cell"] = f64(c[0])
            out["D" if self._md.get("relax") else "eta"] = e[0]
        if results:
            F = packed[:3 * N].reshape(N, 3).copy()
            stress = np.zeros(6)
            check(_lib.load().sgpr_stress_from_virial(ptr(f64(packed[4 * N + 1:4 * N + 10])), ptr(cell), ptr(stress)))
            out.update(forces=F, beta=packed[3 * N:4 * N].copy(), energy=float(packed[4 * N]), stress=stress)
            if self._md.get("relax"):
                out["velocities"] = v.copy()
            elif self._md.get("nh"):   # Nose-Hoover: the centred velocity of this configuration (v is the one before it)
                vn = np.empty((N, 3))
                check(_lib.load().sgpr_md_velocities(self._h, ptr(vn)))
                out["velocities"] = vn
            else:
                Fk = F
                if pend.value and self._md.get("shrink") is not None and which == 0:   # (the kick the filtered integrator gives)
                    Fk = F - np.clip(self.md_filter_state()[0] * self._md["shrink"], -1.0, 1.0)
                out["velocities"] = v + self._md["hdt"] * Fk / self._md["masses"][:, None] if pend.value else v.copy()
                if self._md.get("fixed") is not None:   # (a held component: the integrator's F = 0, v = 0)
                    out["velocities"] = np.where(self._md["fixed"], 0.0, out["velocities"])
        return out

    def md_record(self, every, velocities=True, results=True):
        """Record every `every`-th configuration of the run (trajectory index n with n % every == 0) from the next md_run on,
        without cutting the run: behind the evaluation of such a configuration one extra launch copies it into a record in
        device memory, in caller atom order (sgpr_md_record; a trajectory writer's loginterval, cl/md.py:24-26).  Positions
        always; velocities: what the integrator holds (md_state's velocities_pre); results: forces, covloss, energy, virial.
        every = 0: off.  After md_begin / relax_begin, between any two md_run calls; md_frames() fetches a call's frames."""
        check(_lib.load().sgpr_md_record(self._h, int(every), (1 if velocities else 0) | (2 if results else 0)))
        self._md["record"] = (int(every), bool(velocities), bool(results)) if every else None

    def md_frame_count(self):
        """Frames of the last md_run that stand (sgpr_md_frame_count)."""
        k = C.c_int(0)
        check(_lib.load().sgpr_md_frame_count(self._h, C.addressof(k)))
        return k.value

    def md_frames(self, closed=True, reuse=False):
        """The frames the last md_run recorded, as md_state would have returned them had the run been cut behind each (the
        same bits): dict(index [k], positions [k, N, 3]); velocities_pre [k, N, 3] where velocities were recorded; where
        results were: forces, beta, energy (views of the one packed array fetched), stress (of the frame's own cell) and, for
        Langevin / velocity Verlet with closed=True, velocities — the closing half kick applied, md_state(results=True)'s
        expression, held components zero (three passes over [k, N, 3] on the host: closed=False leaves it out).  Moving-cell
        runs and relaxations: cell, and eta or D, from md_cells' rows of the same evaluations.  The frame of an evaluation the
        covloss gate halted is not among them: the next call records that configuration again.  One device-to-host copy per
        array, nothing is un-permuted on the host.  reuse=True: the arrays are views of buffers the model keeps and fills again
        at the next md_frames(reuse=True) — a caller that is done with a call's frames before it fetches the next call's
        (a 256-frame call of 4096 atoms is 84 MB: fresh pages every call cost as much as the copy)."""
        N, k = self._md["N"], self.md_frame_count()
        if k == 0:
            check(_lib.load().sgpr_md_frames(self._h, 0, 1, None, None, None, None))   # (SGPR_E_INVALID: the call recorded nothing)
        _, want_v, want_r = self._md["record_call"]

        def room(key, shape):
            if not reuse:
                return np.empty((k,) + shape)
            buf = self._md.setdefault("frame_bufs", {})
            if key not in buf or len(buf[key]) < k or buf[key].shape[1:] != shape:
                buf[key] = np.empty((k,) + shape)
            return buf[key][:k]
        idx = np.zeros(k, dtype=np.int64)
        x = room("x", (N, 3))
        v = room("v", (N, 3)) if want_v else None
        packed = room("p", (4 * N + 11,)) if want_r else None
        check(_lib.load().sgpr_md_frames(self._h, 0, k, ptr(idx), ptr(x), ptr(v), ptr(packed)))
        out = dict(index=idx, positions=x)
        if want_v:
            out["velocities_pre"] = v
        cells = None
        if self._md.get("npt"):
            t0, done = self._md["run"]
            c, e = self.md_cells(t0, done)
            cells = out["cell"] = c[idx - t0]
            out["D" if self._md.get("relax") else "eta"] = e[idx - t0]
        if want_r:
            out["forces"] = packed[:, :3 * N].reshape(k, N, 3)
            out["beta"] = packed[:, 3 * N:4 * N]
            out["energy"] = packed[:, 4 * N]
            stress, vir = np.zeros((k, 6)), f64(packed[:, 4 * N + 1:4 * N + 10])
            for r in range(k):
                cell = self._md["cell"] if cells is None else f64(cells[r])
                check(_lib.load().sgpr_stress_from_virial(ptr(vir[r]), ptr(cell), ptr(stress[r])))
            out["stress"] = stress
            # (a filtered run, md_begin(ml_filter=): the kick is the filtered force's and the record holds no accumulators — left out)
            if closed and want_v and not self._md.get("relax") and not self._md.get("nh") and self._md.get("shrink") is None:
                # v + hdt * F / m, operation by operation as md_state spells it (every configuration but the start of the
                # trajectory has a half kick pending), in one array
                vel = np.multiply(self._md["hdt"], out["forces"])
                np.divide(vel, self._md["masses"][:, None], out=vel)
                np.add(v, vel, out=vel)
                vel[idx == 0] = v[idx == 0]
                if self._md.get("fixed") is not None:   # (a held component: the integrator's F = 0, v = 0)
                    vel[:, self._md["fixed"]] = 0.0
                out["velocities"] = vel
        return out

    def _md_species(self, n=None):
        """The `species` and `n` entries of an accumulator's table: the model's table and its atoms in the run's frame — as the
        library reports them, or (None) counted from the run's numbers."""
        if n is None:
            numbers = np.asarray(self._md["numbers"])
            n = [int(np.sum(numbers == int(z))) for z in self.species]
        return dict(species=np.array([int(z) for z in self.species]), n=np.array(n))

    def md_msd(self, every, levels, com=False):
        """Accumulate mean-square displacements inside the loop (sgpr_md_msd; md_msd.inc has the scheme, workloads.MsdBlocks is
        the host twin and the definition): configuration n with n % every == 0 is sample n / every; level l < levels has the
        lag 2^l samples, one origin and windows that do not overlap, and per species of the model's table gains the tracer
        msd = mean |d_i - c|^2 and the collective smd = |sum (d_i - c)|^2 / n_z of every window (c: the displacement of the
        frame's centre of mass with com=True, else 0) — what theforce/analysis/analysis.py's `correlator` works out of a stored
        trajectory.  After md_begin, before the first md_run; every = 0 detaches and frees.  md_msd_table() reads the table.  Langevin,
        velocity Verlet and Nose-Hoover at constant cell on one rank, with or without fixed=, ml_filter=, md_meta and md_record;
        a barostat, a committee, a relaxation, a band, a polymer and several ranks: NotImplementedError."""
        _attach(_lib.load().sgpr_md_msd(self._h, int(every), int(levels), 1 if com else 0))
        self._md["msd"] = (int(every), int(levels)) if every else None

    def md_msd_table(self):
        """The table of md_msd as it stands (sgpr_md_msd_read; between two md_run calls): dict(lags [L] in evaluations,
        count [L] windows per level, msd, msd_sq, smd, smd_sq [L, S] the sums over a level's windows per species, species [S]
        the model's table, n [S] its atoms in the frame, samples, next_due)."""
        if not self._md.get("msd"):
            raise RuntimeError("md_msd_table: no accumulator on this run (md_msd)")
        every, L = self._md["msd"]
        S = len(self.species)
        tab, cnt, info = np.zeros((L, S, 4)), np.zeros(L, dtype=np.int64), np.zeros(2, dtype=np.int64)
        check(_lib.load().sgpr_md_msd_read(self._h, ptr(tab), ptr(cnt), ptr(info)))
        return dict(lags=every * 2 ** np.arange(L, dtype=np.int64), count=cnt, msd=tab[:, :, 0].copy(), msd_sq=tab[:, :, 1].copy(),
                    smd=tab[:, :, 2].copy(), smd_sq=tab[:, :, 3].copy(), samples=int(info[0]), next_due=int(info[1]), **self._md_species())

    def md_rdf(self, every, rmax, bins=100, rmin=0.0):
        """Accumulate radial distribution functions inside the loop (sgpr_md_rdf; md_rdf.inc has the scheme, workloads.RdfCounts
        is the host twin and the definition): behind the evaluation of every configuration n with n % every == 0 the distances
        rmin <= r < rmax of all pairs — periodic images and self-images included; rmax may exceed the model's cutoff and half
        the cell — are counted into `bins` bins per pair of species of the model's table, as integers: what
        theforce/analysis/rdf.py's `rdf` works out of a stored trajectory.  After md_begin, before the first md_run; every = 0
        detaches.  md_rdf_table() reads the counts, transport.radial_distribution forms g(r).  Langevin, velocity Verlet and
        Nose-Hoover at constant cell on one rank, with or without fixed=, ml_filter=, md_meta, md_record and md_msd; a barostat,
        a committee, a relaxation, a band, a polymer, several ranks and an rmax beyond 2.5 cell heights: NotImplementedError."""
        _attach(_lib.load().sgpr_md_rdf(self._h, int(every), float(rmin), float(rmax), int(bins)))
        self._md["rdf"] = (int(every), int(bins)) if every else None

    def md_rdf_table(self):
        """The table of md_rdf as it stands (sgpr_md_rdf_read; between two md_run calls): dict(hist [S, S, bins] uint64 the
        counts per ordered pair of species slots (symmetric), species [S] the model's table, n [S] its atoms in the frame,
        samples, next_due, every, bins, rmin, rmax, volume)."""
        if not self._md.get("rdf"):
            raise RuntimeError("md_rdf_table: no accumulator on this run (md_rdf)")
        every, bins = self._md["rdf"]
        S = len(self.species)
        hist, info, geom = np.zeros((S, S, bins), dtype=np.uint64), np.zeros(4 + S, dtype=np.int64), np.zeros(3)
        check(_lib.load().sgpr_md_rdf_read(self._h, ptr(hist), ptr(info), ptr(geom)))
        return dict(hist=hist, samples=int(info[0]), next_due=int(info[1]), every=every, bins=int(info[2]), rmin=float(geom[1]),
                    rmax=float(geom[2]), volume=float(geom[0]), **self._md_species(info[4:]))

    def md_vacf(self, every, lags, origin_every=1, com=False):
        """Accumulate velocity autocorrelations inside the loop (sgpr_md_vacf; md_vacf.inc has the scheme, workloads.VacfRing is
        the host twin and the definition): configuration n with n % every == 0 is sample n / every, its velocity the one
        md_state(results=True)["velocities"] shows; for every lag k < lags and origin o = s - k with o % origin_every == 0, per
        species of the model's table, the tracer correlation mean_i (v_i(s) - c_s).(v_i(o) - c_o) and the collective block
        e_a(s).e_b(o) of the species' currents (c: the velocity of the frame's centre of mass with com=True, else 0) are added
        to a table.  A sample is stored behind its evaluation and correlated when the next one arrives: the last one of a run is
        pending.  After md_begin, before the first md_run; every = 0 detaches.  md_vacf_table() reads the table.  Langevin,
        velocity Verlet and Nose-Hoover at constant cell on one rank, with or without fixed=, md_record, md_msd and md_rdf; a
        barostat, a committee, a relaxation, a band, a polymer, several ranks, ml_filter= and md_meta (their closing kick uses
        a force other than the packed one), more than 8192 lags or a ring (lags + 1) * 24 N over 4 GiB: NotImplementedError."""
        _attach(_lib.load().sgpr_md_vacf(self._h, int(every), int(lags), int(origin_every), 1 if com else 0))
        self._md["vacf"] = (int(every), int(lags)) if every else None

    def md_vacf_table(self):
        """The table of md_vacf as it stands (sgpr_md_vacf_read; between two md_run calls): dict(tracer [lags, S], collective
        [lags, S, S] the sums over the pairs (s, o) of a lag, count [lags] their number, lags [lags] in configurations, species [S]
        the model's table, n [S] its atoms in the frame, samples (correlated), pending (0 / 1), next_due)."""
        if not self._md.get("vacf"):
            raise RuntimeError("md_vacf_table: no accumulator on this run (md_vacf)")
        every, L = self._md["vacf"]
        S = len(self.species)
        tr, col, cnt, info = np.zeros((L, S)), np.zeros((L, S, S)), np.zeros(L, dtype=np.int64), np.zeros(3 + S, dtype=np.int64)
        check(_lib.load().sgpr_md_vacf_read(self._h, ptr(tr), ptr(col), ptr(cnt), ptr(info)))
        return dict(tracer=tr, collective=col, count=cnt, lags=every * np.arange(L, dtype=np.int64), samples=int(info[0]),
                    pending=int(info[1]), next_due=int(info[2]), **self._md_species(info[3:]))

    def md_vanhove(self, every, levels, rmax, rbins, tbins=1, pbins=1, dmax=None, dbins=0):
        """Accumulate van Hove correlation functions inside the loop (sgpr_md_vanhove; md_vanhove.inc has the scheme,
        workloads.VanHoveCounts is the host twin and the definition; all entries are counts, the two are equal).  Samples and
        levels as md_msd: configuration n with n % every == 0 is sample n / every; level l < levels has the lag 2^l samples,
        one origin and windows that do not overlap.  Self part: per species of the model's table the histogram of the atoms'
        raw displacements over (r < rmax, theta, phi) in rbins x tbins x pbins bins — what
        theforce/analysis/analysis.py's `hist_rtp_displacements` takes from a stored trajectory at one lag; tbins = pbins = 1 is
        the radial G_s(r, t); displacements of rmax and more are counted in `over`.  Distinct part (dbins > 0): per ordered pair
        of species the distances r < dmax between an atom's origin and the other atoms' present positions, periodic images
        included (the atom's own image at shift 0 left out), in dbins bins.  After md_begin, before the first md_run; every = 0
        detaches and frees.  md_vanhove_table() reads the tables.  Langevin, velocity Verlet and Nose-Hoover at constant cell on
        one rank, with or without fixed=, ml_filter=, md_meta, md_record, md_msd, md_rdf and md_vacf; a barostat, a committee, a
        relaxation, a band, a polymer, several ranks, a self table over 1 GiB and a dmax beyond 2.5 cell heights:
        NotImplementedError."""
        from .workloads import vanhove_edges
        lib = _lib.load()
        _attach(lib.sgpr_md_vanhove(self._h, int(every), int(levels), float(rmax), int(rbins), int(tbins), int(pbins),
                                    float(dmax) if dbins else 0.0, int(dbins)))
        if every:   # (the edges the twin compares with: numpy's doubles, not this library's)
            ct, cu, su = (np.ascontiguousarray(a, dtype=np.float64) for a in vanhove_edges(tbins, pbins))
            check(lib.sgpr_md_vanhove_edges(self._h, ptr(ct), ptr(cu), ptr(su)))
        self._md["vanhove"] = (int(every), int(levels), int(rbins), int(tbins), int(pbins), int(dbins)) if every else None

    def md_vanhove_table(self):
        """The tables of md_vanhove as they stand (sgpr_md_vanhove_read; between two md_run calls): a dict with "self" [L, S, rbins,
        tbins, pbins], over [L, S], distinct [L, S, S, dbins] (origin's species first), all uint64; count [L] windows per level,
        lags [L] in configurations, species [S] the model's table, n [S] its atoms in the frame, samples, next_due, every, levels,
        rmax, rbins, tbins, pbins, dmax, dbins, volume."""
        if not self._md.get("vanhove"):
            raise RuntimeError("md_vanhove_table: no accumulator on this run (md_vanhove)")
        every, L, rbins, tbins, pbins, dbins = self._md["vanhove"]
        S = len(self.species)
        hs, over, hd = (np.zeros(shape, dtype=np.uint64) for shape in ((L, S, rbins, tbins, pbins), (L, S), (L, S, S, dbins)))
        cnt, info, geom = np.zeros(L, dtype=np.int64), np.zeros(8 + S, dtype=np.int64), np.zeros(3)
        check(_lib.load().sgpr_md_vanhove_read(self._h, ptr(hs), ptr(over), ptr(hd) if dbins else None, ptr(cnt), ptr(info), ptr(geom)))
        tab = dict(over=over, distinct=hd, count=cnt, lags=every * 2 ** np.arange(L, dtype=np.int64), samples=int(info[0]),
                   next_due=int(info[1]), every=every, levels=L, rmax=float(geom[1]), rbins=rbins, tbins=tbins, pbins=pbins,
                   dmax=float(geom[2]), dbins=dbins, volume=float(geom[0]), **self._md_species(info[8:]))
        tab["self"] = hs
        return tab

    def md_adf(self, every, bins=180, cutoffs=None):
        """Accumulate bond-angle and coordination distributions inside the loop (sgpr_md_adf; md_adf.inc has the scheme,
        workloads.AdfCounts is the host twin and the definition; all entries are counts, the two are equal).  `cutoffs`: the bond
        cutoffs, a scalar (all pairs) or a dict {(Z1, Z2): r} over the model's species (pairs that are absent never bond), each
        at most the model's cutoff.  Behind the evaluation of every configuration n with n % every == 0, for every centre the
        angles between all pairs of its neighbours within the cutoffs — periodic images and self-images included, read from the
        neighbour list the step has just built — are counted into `bins` bins over [0, pi] per (centre, end, end) of species, and
        its number of neighbours per species into 64 bins (the last: 63 and above).  After md_begin, before the first md_run;
        every = 0 detaches and frees.  md_adf_table() reads the tables; transport.angle_distribution and transport.coordination
        form P(theta) and P(n).  Langevin, velocity Verlet and Nose-Hoover at constant cell on one rank, with or without fixed=,
        ml_filter=, md_meta, md_record, md_msd, md_rdf, md_vacf and md_vanhove; a barostat, a committee, a relaxation, a band, a
        polymer, several ranks and a cutoff beyond the model's: NotImplementedError."""
        from .workloads import adf_cutoffs, adf_edges
        lib = _lib.load()
        if not every:
            check(lib.sgpr_md_adf(self._h, 0, 0, None, None))
            self._md["adf"] = None
            return
        if cutoffs is None:
            raise ValueError("md_adf: cutoffs= (a scalar or {(Z1, Z2): r}) says which pairs bond")
        species = [int(z) for z in self.species]
        cut = np.ascontiguousarray(adf_cutoffs(cutoffs, species), dtype=np.float64)
        if cut.shape != (len(species), len(species)):
            raise ValueError(f"md_adf: the cutoff table is [{len(species)}, {len(species)}] over the model's species")
        if not 1 <= int(bins) <= 1024:
            raise ValueError("md_adf: 1 <= bins <= 1024")
        ct = np.ascontiguousarray(adf_edges(bins), dtype=np.float64)
        _attach(lib.sgpr_md_adf(self._h, int(every), int(bins), ptr(cut), ptr(ct)))
        self._md["adf"] = (int(every), int(bins), cut)

    def md_adf_table(self):
        """The tables of md_adf as they stand (sgpr_md_adf_read; between two md_run calls): dict(angles [S, S, S, bins] uint64 the
        counts per (centre, end, end) of species slots (symmetric in the ends), coord [S, S, 64] uint64 per (centre, neighbour)
        the centres with n neighbours, species [S] the model's table, n [S] its atoms in the frame, samples, next_due, every,
        bins, cut [S, S])."""
        if not self._md.get("adf"):
            raise RuntimeError("md_adf_table: no accumulator on this run (md_adf)")
        every, bins, cut = self._md["adf"]
        S = len(self.species)
        angles, coord, info = np.zeros((S, S, S, bins), dtype=np.uint64), np.zeros((S, S, 64), dtype=np.uint64), np.zeros(4 + S, dtype=np.int64)
        check(_lib.load().sgpr_md_adf_read(self._h, ptr(angles), ptr(coord), ptr(info)))
        return dict(angles=angles, coord=coord, samples=int(info[0]), next_due=int(info[1]), every=every, bins=int(info[2]), cut=cut.copy(),
                    **self._md_species(info[4:]))

    def md_sq(self, every, hkl=None, lags=1, origin_every=1):
        """Accumulate partial structure factors and coherent intermediate scattering functions inside the loop (sgpr_md_sq;
        md_sq.inc has the scheme and the accuracy bound, workloads.SqRing is the host twin and the definition).  `hkl`: int
        [nq, 3] vectors of the reciprocal lattice of the run's cell, q_j = 2 pi hkl_j inv(cell)^T (transport.q_vectors lists a
        half-sphere of them), one of each +- pair, every |index| <= 32.  Configuration n with n % every == 0 is sample n / every:
        per species of the model's table the density rho_z(q_j) = sum_z exp(i q_j . r_i) is formed, added to `mean`, kept in a
        ring of `lags` samples, and for every lag k < lags whose origin o = s - k has o % origin_every == 0 the S x S block
        Re(rho_a(s) conj rho_b(o)) is added to f[k, j].  After md_begin, before the first md_run; every = 0 detaches and frees.
        md_sq_table() reads the tables; transport.structure_factor, intermediate_scattering and dynamic_structure_factor read
        those.  Langevin, velocity Verlet and Nose-Hoover at constant cell on one rank, with or without fixed=, ml_filter=,
        md_meta, md_record and the other accumulators; a barostat, a committee, a relaxation, a band, a polymer, several ranks
        and tables over 1 GiB: NotImplementedError."""
        lib = _lib.load()
        if not every:
            check(lib.sgpr_md_sq(self._h, 0, 0, None, 0, 0))
            self._md["sq"] = None
            return
        if hkl is None:
            raise ValueError("md_sq: hkl= (int [nq, 3]; transport.q_vectors) names the wave vectors")
        given = np.asarray(hkl)
        if given.ndim != 2 or given.shape[1] != 3 or not np.array_equal(given, np.rint(given)):
            raise ValueError("md_sq: hkl is an integer array [nq, 3]")
        hkl = np.ascontiguousarray(given, dtype=np.int32)
        _attach(lib.sgpr_md_sq(self._h, int(every), len(hkl), ptr(hkl), int(lags), int(origin_every)))
        self._md["sq"] = (int(every), hkl.astype(np.int64), int(lags), int(origin_every))

    def md_sq_table(self):
        """The tables of md_sq as they stand (sgpr_md_sq_read; between two md_run calls): dict(f [lags, nq, S, S] the sums of
        Re(rho_a(s) conj rho_b(s - k)) over the pairs of a lag, mean [nq, S] complex the sum of rho over the samples, count
        [lags] the pairs, lags [lags] in configurations, hkl [nq, 3], q [nq, 3] = 2 pi hkl inv(cell)^T, species [S] the model's
        table, n [S] its atoms in the frame, origin_every, samples, next_due)."""
        if not self._md.get("sq"):
            raise RuntimeError("md_sq_table: no accumulator on this run (md_sq)")
        from .workloads import sq_vectors
        every, hkl, L, origin_every = self._md["sq"]
        S, nq = len(self.species), len(hkl)
        f, mean, cnt, info = np.zeros((L, nq, S, S)), np.zeros((nq, S, 2)), np.zeros(L, dtype=np.int64), np.zeros(2 + S, dtype=np.int64)
        check(_lib.load().sgpr_md_sq_read(self._h, ptr(f), ptr(mean), ptr(cnt), ptr(info)))
        return dict(f=f, mean=mean[:, :, 0] + 1j * mean[:, :, 1], count=cnt, lags=every * np.arange(L, dtype=np.int64), hkl=hkl.copy(),
                    q=sq_vectors(hkl, self._md["cell"]), origin_every=origin_every, samples=int(info[0]), next_due=int(info[1]), **self._md_species(info[2:]))

    def md_committee(self, members, moving_cell=None):
        """The Bayesian committee of the run just begun (sgpr_md_committee; calculator_bcm.py has the rule): `members`, frozen
        SGPRModels with weights and choli on this model's device, are evaluated beside this (live) model at every
        configuration of md_run, in the order given with this model last — the run integrates the weighted forces, gates on
        the largest member-wise minimum covloss, and its rows and md_state(results=True) carry the committee's energy,
        forces, stress and covloss.  After md_begin (and its thermostat), before the first md_run; an empty list detaches.
        Langevin, velocity Verlet and Nose-Hoover at constant cell, and — moving_cell=True: the run's option "md_committee_cell",
        without which a run with a barostat refuses a committee as before — Nose-Hoover with a barostat (md_begin(pfactor=): every
        member is evaluated in the cell of the configuration, the moving cell integrates the committee's stress, md_cells() and
        md_state() return the cell as for a single model); one rank, no mask, no filter, no bias, no frame record.  The model
        keeps references to the members until md_end, the next md_begin or a detach."""
        members = list(members or ())
        if moving_cell is not None:   # (the run's option: md_begin switches it off again)
            check(_lib.load().sgpr_set_option(self._h, b"md_committee_cell", 1 if moving_cell else 0))
        arr = (C.c_void_p * max(len(members), 1))(*[None if mm is None else mm._h.value for mm in members])
        check(_lib.load().sgpr_md_committee(self._h, len(members), arr if members else None))
        self._md["members"] = members

    def md_committee_info(self):
        """(w [K + 1], covmax [K + 1]) — the weights and the largest covlosses of the members in their order, this model last —
        of the last evaluation whose results stand (sgpr_md_committee_info)."""
        K1 = len(self._md.get("members") or ()) + 1
        w, cm = np.zeros(K1), np.zeros(K1)
        check(_lib.load().sgpr_md_committee_info(self._h, ptr(w), ptr(cm)))
        return w, cm

    def md_end(self):
        check(_lib.load().sgpr_md_end(self._h))
        if getattr(self, "_md", None):
            self._md.pop("members", None)

    def descriptors(self, N):
        S, D = len(self.species), (self.nmax + 1) ** 2 * (self.lmax + 1)
        out = np.zeros((N, S, S, D))
        check(_lib.load().sgpr_get_descriptors(self._h, ptr(out)))
        return out

    def neighbors(self, N):
        p = np.zeros(N + 1, np.int64)
        check(_lib.load().sgpr_get_neighbors(self._h, ptr(p), None, None))
        j = np.zeros(int(p[-1]), np.int32)
        off = np.zeros((int(p[-1]), 3), np.int32)
        check(_lib.load().sgpr_get_neighbors(self._h, ptr(p), ptr(j), ptr(off)))
        return p, j, off

    def last_cov(self, N):
        """K_nm [N, m] of the last evaluated frame, downloaded on demand."""
        out = np.zeros((N, self.m))
        if self.m:
            check(_lib.load().sgpr_get_cov(self._h, int(N), int(self.m), ptr(out)))
        return out

    def local(self, atom):
        """The LCE of one atom of the last evaluated frame (TorchAtoms.local, descriptor/atoms.py:365-382)
        straight from the device neighbour list."""
        nn = C.c_int32(0)
        lib = _lib.load()
        check(lib.sgpr_get_local(self._h, int(atom), C.addressof(nn), None, None, 0))
        z, r = np.zeros(nn.value, np.int32), np.zeros((nn.value, 3))
        check(lib.sgpr_get_local(self._h, int(atom), C.addressof(nn), ptr(z), ptr(r), nn.value))
        return z, r

    def profile(self, on=True):
        check(_lib.load().sgpr_profile(self._h, int(bool(on))))

    def stage_times(self):
        ms = np.zeros(32)
        names = C.create_string_buffer(1024)
        n = _lib.load().sgpr_get_stage_times(self._h, ptr(ms), 32, C.addressof(names), 1024)
        return dict(zip(names.value.decode().split(";"), ms[:n])) if n > 0 else {}
