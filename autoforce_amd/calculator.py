"""ActiveCalculator — the reference's ASE-calculator surface for the SGPR path, backed by
libsgpr_hip (MI355X).  Mirrors theforce/calculator/active.py:

  :104-135   constructor keywords               :425-535   calculate / post_calculate
  :548-611   results (E, F, stress)             :612-640   initiate_model / get_unique_lces
  :642-676   sample_rand_lces                   :706-768   _exact / snapshot / head
  :781-804   covloss                            :806-839   update_lce
  :841-885   update_inducing                    :887-933   update_data
  :942-984   update                             :989-1053  include_data / include_tape
  :1055-1098 build

All numerics (neighbour list, descriptors, K_nm, forces, covloss, training rows, K_mm edits,
Cholesky/QR) run on the device through `SGPRModel`; this file is the control flow and the
acceptance thresholds.  With `calculator=None` it is a pure evaluator; with a teacher
(`calculator=` any ASE-style calculator giving energy/forces/stress) it learns on the fly.

Works with real ASE when installed; otherwise with the minimal shim in autoforce_amd.ase_shim.
"""
import datetime
import os
import time

import numpy as np

try:  # pragma: no cover - ASE is absent from the build image
    from ase.calculators.calculator import Calculator, all_changes
    from ase.calculators.singlepoint import SinglePointCalculator
    from ase.units import GPa, kcal, mol
    kcal_mol = kcal / mol
    HAVE_ASE = True
except ImportError:
    from .ase_shim import Calculator, SinglePointCalculator, all_changes, kcal_mol
    GPa = 1.0 / 160.21766208
    HAVE_ASE = False

from .device_loop import batches, first_on_host, hand_over, held, log_rows, put_state, record_cap, recorded_frames, sync_cap
from .model import Local, SGPRModel
from .posterior import EPS, Frame, PosteriorPotential
from .sgprio import SgprIO
from .sharding import pack_partial, rank_of_atoms, unpack_total

inf = float("inf")


def default_kernel(lmax=3, nmax=3, exponent=4, cutoff=6.0, species=None, device=0, wildcard=False):
    """theforce/calculator/active.py:28-38.  Without `species`: the wildcard SeSoapKernel(lmax, nmax, exponent, cutoff,
    radii=DefaultRadii()) — the reference indexes a fixed 120-wide table, the device layout is dense over the species
    met so far (`wildcard=True` with the current table).  With `species`: the reference builds ONE SubSeSoapKernel per
    listed species and sums them; the only place where that differs from one kernel over the same table is the
    lone-atom term, added once per kernel object (SGPRModel's `lone_weight`)."""
    return SGPRModel(lmax, nmax, exponent, cutoff, species=species, device=device,
                     lone_weight=1 if wildcard or not species else len(species))


class Switch:
    """active.py:82-101: a threshold that depends on the largest force of the frame:
    Switch([v0, s1, v1, s2, v2]) is v0 below s1, v1 between s1 and s2, v2 above."""

    def __init__(self, value):
        self._value = value
        seq = list(value) if hasattr(value, "__iter__") else [value]
        self.switches = (-inf, *seq[1::2], inf)
        self.values = seq[0::2]
        if any(a > b for a, b in zip(self.switches, self.switches[1:])):
            raise RuntimeError("Switch is not ordered!")

    def __repr__(self):
        return f"{self._value}"

    def __call__(self, x):
        k = 0
        for k, (lo, hi) in enumerate(zip(self.switches, self.switches[1:])):
            if lo < x < hi:
                break
        return self.values[k]


def _switched(name):
    def get(self):
        return getattr(self, "_" + name)(self.maximum_force)

    def put(self, value):
        setattr(self, "_" + name, value if isinstance(value, Switch) else Switch(value))

    return property(get, put)


class ActiveCalculator(Calculator):
    implemented_properties = ["energy", "forces", "stress", "free_energy"]
    ediff, ediff_lb, ediff_ub, fdiff = (_switched(n) for n in ("ediff", "ediff_lb", "ediff_ub", "fdiff"))

    def __init__(self, covariance=None, calculator=None, process_group=None, meta=None, logfile="active.log",
                 pckl=None, tape=None, test=None, stdout=False, ediff=2 * kcal_mol, ediff_lb=None, ediff_ub=None,
                 ediff_tot=4 * kcal_mol, fdiff=3 * kcal_mol, noise_f=kcal_mol, ioptim=1, max_data=inf,
                 max_inducing=inf, kernel_kw=None, veto=None, include_params=None, eps_dr=0.1, ignore=None,
                 report_timings=False, step0_forced_fp=False, nbeads=1, engine=None):
        """
        covariance:    SGPRModel | PosteriorPotential | path to a saved model (.npz,
                       autoforce_amd.modelio) | None (+ kernel_kw with a `species` entry -> empty model)
        calculator:    None (evaluate only) | teacher: any ASE-style calculator (energy/forces/stress)
        process_group: None | torch.distributed process group over which atoms are sharded
        pckl:          None | path of the .npz the model is saved to after every update
        tape:          None | path of the .sgpr tape that accepted data / LCEs are appended to
        engine:        test hook — an object with SGPRModel's methods
        The remaining keywords have the reference's meaning (active.py:137-287).
        """
        Calculator.__init__(self)
        self._calc = calculator
        self.process_group = process_group
        self.pckl = pckl
        self.maximum_force = inf
        self.logfile, self.stdout, self._logpref = logfile, stdout, ""
        self.step = 0
        self._wildcard = False
        self._comm_note, self._hello = "", False
        self._peer_atoms = 0
        self._sys_cache = None
        self.get_model(engine if engine is not None else covariance, kernel_kw or {})
        self.ediff = ediff
        self.ediff_lb = ediff_lb or ediff
        self.ediff_ub = ediff_ub or ediff
        self.ediff_tot, self.fdiff, self.noise_f = ediff_tot, fdiff, noise_f
        self.ioptim, self._ioptim = ioptim, 0
        self.max_data, self.max_inducing = max_data, max_inducing
        self.meta = meta
        self.log("active calculator says Hello!", mode="w")
        self._hello = True
        if self._comm_note:
            self.log(self._comm_note)
        self.log_settings()
        self.log("model size: {} {}".format(*self.size))
        self.tape = None if tape is None else SgprIO(tape, rank=self.rank)
        self.test, self._last_test, self._ktest = test, 0, 0
        self.updated = False
        self._update_args = {}
        self._veto = {} if veto is None else dict(veto)
        self.include_params = {"fmax": inf}
        self.include_params.update(include_params or {})
        self.tune_for_md = True
        self.eps_dr = eps_dr
        self.ignore = [] if ignore is None else list(ignore)
        self.report_timings = report_timings
        self.step0_forced_fp = step0_forced_fp
        self.nbeads = nbeads
        self.deltas, self.covlog, self._cov = None, "", None
        self._cov_gen = None
        self.blind = False
        self._saved_for_tape = None
        self._beta = None
        self._nl = None
        if self.nbeads > 1:
            self.log(f"You are going quantum (PIMD)! Number of beads: {self.nbeads}")

    # ------------------------------------------------------------------ model plumbing
    def get_model(self, model, kernel_kw):
        """active.py:338-362."""
        if isinstance(model, str):
            from .modelio import load_model
            model = load_model(model)
        elif model is None:
            if self.pckl and os.path.isfile(self.pckl):
                from .modelio import load_model
                model = load_model(self.pckl)
            else:
                kw = dict(kernel_kw)
                if not kw.get("species"):
                    # the reference's default kernel is the species-wildcard one (active.py:28-38): the table
                    # starts with the first frame's species and grows when a new one turns up (_ensure_species)
                    self._wildcard = True
                    kw["species"] = [0]  # placeholder, replaced before the first evaluation
                    kw["wildcard"] = True
                model = default_kernel(**kw)
        if not isinstance(model, PosteriorPotential):
            model = PosteriorPotential(model)
        model._sync = self._broadcast if self.process_group is not None else None
        self.model = model
        self._attach_native_comm()

    def _attach_native_comm(self):
        """Sharded frames on the HIP engine: the ranks' partial sums are combined inside the library
        by ONE RCCL all-reduce on the step's stream (sgpr_comm_init); the process group only carries
        the 128-byte id during set-up.  Engines without that entry point (the CPU oracle engine of the
        tests) keep the host-side all-reduce of `_evaluate_engine`."""
        eng = self.model.engine
        if self.process_group is None or not hasattr(eng, "comm_init"):
            return
        import torch.distributed as dist
        rank, world = self._dist()
        if world < 2:
            return
        # SGPR_COLLECTIVE = auto (default): the library's own exchange through hipIpc-mapped buffers (deterministic sums, runs
        # with several ranks on one device, the device MD loop can run sharded on it), else RCCL, else the host-side
        # all-reduce; ipc / rccl / host: only that one (and the host-side all-reduce behind it)
        mode = os.environ.get("SGPR_COLLECTIVE", "auto")
        if mode in ("auto", "ipc") and hasattr(eng, "peer_export") and self._attach_peer(max(self._peer_atoms, 4096)):
            return
        if mode in ("ipc", "host"):
            return
        # every rank takes the same branch: the outcome is agreed on (MIN over ranks) before anybody evaluates.  A rank
        # that cannot build the communicator (RCCL missing; two ranks on one device — RCCL refuses duplicate GPUs)
        # must not leave the others inside ncclCommInitRank: the id travels first, the attempt is made by all, and on
        # any failure all fall back to the host-side all-reduce of `_evaluate_engine`.
        import torch
        ok = 1
        try:
            box = [eng.comm_unique_id() if rank == 0 else None]
        except Exception as exc:  # noqa: BLE001
            box, ok = [None], 0
            self._comm_note = f"native communicator unavailable on rank 0: {exc}"
        dist.broadcast_object_list(box, src=dist.get_global_rank(self.process_group, 0), group=self.process_group)
        if box[0] is None:
            ok = 0
        else:
            try:
                from .watchdog import Watchdog
                with Watchdog("sgpr_comm_init (ncclCommInitRank)", rank=rank):
                    eng.comm_init(box[0], rank, world)
            except Exception as exc:  # noqa: BLE001
                ok = 0
                self._comm_note = f"native communicator not built ({exc}): host-side all-reduce instead"
        if self._min_over_ranks(ok) == 0:
            if getattr(eng, "comm_world", 1) > 1:
                eng.comm_destroy()
            if not self._comm_note:
                self._comm_note = "native communicator not built on another rank: host-side all-reduce instead"
        if self._comm_note and self._hello:
            self.log(self._comm_note)

    def _attach_peer(self, atoms_cap):
        """The library's own exchange (SGPRModel.peer_export / peer_attach) for frames of up to `atoms_cap` atoms: every rank
        exports its receive buffers, the handles travel over the process group, everybody maps everybody's.  The outcome is
        agreed on (MIN over the ranks): all attached, or nobody."""
        import torch
        import torch.distributed as dist
        eng = self.model.engine
        rank, world = self._dist()
        ok, blob, why = 1, None, ""
        try:
            blob = eng.peer_export(rank, world, 7 * int(atoms_cap) + 11)
        except Exception as exc:  # noqa: BLE001
            ok, why = 0, str(exc)
        blobs = [None] * world
        dist.all_gather_object(blobs, blob, group=self.process_group)
        if ok and all(b is not None for b in blobs):
            try:
                eng.peer_attach(blobs)
            except Exception as exc:  # noqa: BLE001
                ok, why = 0, str(exc)
        else:
            ok = 0
        # every rank tries the exchange once before anybody relies on it (collective: all ranks that attached take part)
        if self._min_over_ranks(ok) == 1 and not eng.peer_selftest(rank, world):
            ok, why = 0, "the self-test exchange did not return the expected sum"
        if self._min_over_ranks(ok) == 0:
            if blob is not None:
                eng.peer_destroy()
            self._comm_note = f"the library's own exchange was not built ({why or 'another rank failed'})"
            if self._hello:
                self.log(self._comm_note)
            return False
        self._peer_atoms = int(atoms_cap)
        return True

    def _min_over_ranks(self, value):
        """MIN of an integer over the process group (an NCCL / RCCL group reduces device tensors only)."""
        import torch
        import torch.distributed as dist
        t = torch.tensor([int(value)])
        if dist.get_backend(self.process_group) == "nccl":
            t = t.cuda()
        dist.all_reduce(t, op=dist.ReduceOp.MIN, group=self.process_group)
        return int(t.item())

    def _peer_fit(self, engine, N):
        """A frame larger than the buffers of the library's own exchange hold: export and attach again (collective: every
        rank sees the same N and takes the same branch)."""
        world = self._dist()[1]
        if world > 1 and getattr(engine, "peer_world", 1) == world and N > self._peer_atoms and engine is self.engine:
            self._attach_peer(2 * N)

    @property
    def maximum_force(self):
        """max |F| of the frame in `results` (active.py:573-576; what the Switch thresholds depend on), computed when
        somebody asks: a prediction-only step never does."""
        if self._maxf is None:
            f = self.results.get("forces")
            self._maxf = inf if f is None else (float(np.abs(f).max()) if len(f) else 0.0)
        return self._maxf

    @maximum_force.setter
    def maximum_force(self, value):
        self._maxf = value

    @property
    def engine(self):
        return self.model.engine

    @property
    def active(self):
        return self._calc is not None

    @property
    def size(self):
        return self.model.ndata, len(self.model.X)  # active.py:375-376

    @property
    def rank(self):
        return self._dist()[0]

    @property
    def world_size(self):
        return self._dist()[1]

    def _dist(self):
        if self.process_group is None:
            return 0, 1
        import torch.distributed as dist
        return dist.get_rank(self.process_group), dist.get_world_size(self.process_group)

    def _tensor(self, a):
        import torch
        import torch.distributed as dist
        t = torch.from_numpy(np.ascontiguousarray(a))
        return t.cuda() if dist.get_backend(self.process_group) == "nccl" else t

    def _broadcast(self, arrays):
        """rank 0's mu / choli / ridge / mean weights become everyone's (gppotential.py:592-596)."""
        import torch.distributed as dist
        for a in arrays:
            t = self._tensor(a)
            dist.broadcast(t, 0, group=self.process_group)
            a[...] = t.cpu().numpy()

    # ------------------------------------------------------------------ the hot path
    def _system(self, atoms):
        cell = np.asarray(getattr(atoms.cell, "array", atoms.cell), dtype=float).reshape(3, 3)
        # (the int32 copy of the atomic numbers is kept while the frame's numbers array is the same object with the same
        # content: the conversion of 4096 numbers is 2-3 us of a 130-us step)
        src = atoms.numbers
        c = self._sys_cache
        if c is None or c[0] is not src or len(c[1]) != len(src):   # (the calculator's copy of the atoms keeps ONE numbers array per system)
            c = self._sys_cache = (src, np.asarray(src, dtype=np.int32))
        return (c[1], np.asarray(atoms.positions, dtype=float), cell, np.asarray(atoms.pbc, dtype=bool))

    def _evaluate_engine(self, engine):
        """One device pass of `engine` over the current atoms (sharded + all-reduced when a process
        group is attached): dict(energy, forces, stress, beta, cov)."""
        numbers, positions, cell, pbc = self._system(self.atoms)
        N = len(numbers)
        rank, world = self._dist()
        if not (engine.m > 0 and engine.mu is not None):
            # an empty model predicts its mean (zeros) and knows nothing: covloss = inf
            return dict(energy=0.0, forces=np.zeros((N, 3)), stress=np.zeros(6), beta=np.full(N, inf), ready=False)
        self._peer_fit(engine, N)
        fast = getattr(engine, "predict_view", None)
        if fast is not None and (world == 1 or getattr(engine, "comm_world", 1) == world):
            # results as views of the buffer the device wrote (valid until the call after next): copied where they are kept
            v = fast(numbers, positions, cell, pbc, rank=rank, world=world)
            out = dict(energy=float(v["energy"]), forces=np.array(v["forces"]), stress=np.array(v["stress"]), beta=np.array(v["beta"]))
        else:
            out = engine.predict(numbers, positions, cell, pbc, rank=rank, world=world, cov=False, beta=True)
        if world > 1 and getattr(engine, "comm_world", 1) == world:
            pass  # the library's own RCCL all-reduce already combined the ranks (totals on every rank)
        elif world > 1:
            import torch.distributed as dist
            v = self._tensor(pack_partial(out, N))
            dist.all_reduce(v, group=self.process_group)  # active.py:562,601,602,777 in one collective
            out = unpack_total(v.cpu().numpy(), N)
        out["ready"] = True
        return out

    @property
    def cov(self):
        """K_nm of the last evaluated frame, [N, m] (this rank's rows) — active.py:464 `self.cov`.
        It stays on the device until somebody looks: N x m doubles per step over PCIe would cost
        more than the step itself."""
        if self._cov is None and self.atoms is not None and self.engine.m > 0:
            eng = self.engine
            gen = getattr(eng, "generation", None)
            if gen is not None and gen != self._cov_gen:
                # the device moved on to other frames since this one was evaluated (training rows, trial
                # models, rattled copies): evaluate the current atoms again rather than hand out the
                # K_nm of whatever frame came last
                numbers, positions, cell, pbc = self._system(self.atoms)
                rank, world = self._dist()
                eng.predict(numbers, positions, cell, pbc, rank=rank, world=world, cov=False, beta=False)
                self._cov_gen = eng.generation
            fetch = getattr(eng, "last_cov", None)
            self._cov = fetch(len(self.atoms)) if fetch else None
        return self._cov

    @cov.setter
    def cov(self, value):
        self._cov = value

    def update_results(self, retain_graph=False, covloss_only=False):
        """active.py:548-611 + :781-804 in one device pass: E, F, stress, covloss, cov.
        covloss_only: refresh `cov` and the covloss after the model changed but leave `results`
        alone — inside update_inducing the reference extends cov by a column and keeps the
        pre-update predictions, which update_data then offers as 'fake' labels."""
        out = self._evaluate_engine(self.engine)
        self._cov = None  # fetched lazily
        self._cov_gen = getattr(self.engine, "generation", None)  # the frame `cov` would be fetched from
        self._nl = None
        self._beta = out["beta"]
        if covloss_only:
            return
        self._set_results(out)

    def _set_results(self, out):
        self.results["energy"] = np.asarray(out["energy"])
        self.results["forces"] = np.asarray(out["forces"])
        self.results["stress"] = np.asarray(out["stress"])
        self._maxf = None   # (maximum_force: computed when somebody asks, from these forces)

    def _ensure_species(self, numbers):
        """Wildcard mode (no `species` in kernel_kw): extend the model's table to the species met."""
        if not self._wildcard:
            return
        have = [z for z in self.engine.species if z != 0]
        new = sorted(set(int(z) for z in numbers) - set(have))
        if new or 0 in self.engine.species:
            table = sorted(set(have) | set(new))
            if len(table) > 16:
                raise RuntimeError(f"{len(table)} species: the device kernels hold at most 16 species slots")
            self.model.retable(table)
            self._attach_native_comm()
            self.log(f"species table -> {table}")

    def calculate(self, atoms=None, properties=("energy",), system_changes=all_changes):
        timings = [time.time()]
        if self.size[1] == 0 and not self.active:
            raise RuntimeError("you forgot to assign a DFT calculator!")  # active.py:429-430
        Calculator.calculate(self, atoms, properties, system_changes)
        self._ensure_species(self.atoms.numbers)
        self.maximum_force = inf
        timings.append(time.time())
        if self._needs_seed():
            self.initiate_model()
            self._update_args = dict(data=False)
        timings.append(time.time())
        self.update_results(self.active or (self.meta is not None))
        timings.append(time.time())
        self.deltas = None
        self.covlog = ""
        if self.active and not self.veto():
            if (self.step + 1) % self.nbeads == 1 or self.nbeads == 1:  # PIMD: only the first bead samples
                pre = dict(self.results)
                m, n = self.update(**self._update_args)
                if n > 0 or m > 0:
                    self.update_results(self.meta is not None)
                    if self.step > 0:
                        self.deltas = {q: self.results[q] - pre[q] for q in ("energy", "forces", "stress")}
        else:
            covloss_max = float(np.max(self.get_covloss())) if len(self.atoms) else 0.0
            self.covlog = f"{covloss_max}"
            if self.rank == 0 and covloss_max > self.ediff:   # (ediff last: a Switch asks for max |F|)
                self._side_file("active_uncertain", self.atoms, None, "a")
        timings.append(time.time())
        self.post_calculate(timings)

    def _needs_seed(self):
        return self.step == 0 and self.active and self.model.ndata == 0  # active.py:458-461

    def post_calculate(self, timings):
        """active.py:504-535."""
        energy = self.results["energy"]
        if self.active and self.test and self.step - self._last_test > self.test:
            self._test()
        meta = ""
        if self.meta is not None:
            energies, kwargs = self.meta(self)
            if energies is not None:
                meta = f"meta: {float(np.sum(energies))}"
                if hasattr(self.meta, "bias"):
                    # a meta.Meta: the bias acts — energy, forces and stress are added to the results as the reference's
                    # reduce(op="+=") does (active.py:510-516, :557-580); any other callable is logged only, as before
                    V, Fb, Sb = self.meta._last
                    self.results["energy"] = np.asarray(self.results["energy"] + V)
                    self.results["forces"] = self.results["forces"] + Fb
                    self.results["stress"] = self.results["stress"] + Sb
                    self._maxf = None
                    energy = self.results["energy"]
        if (self.logfile or self.stdout) and self.rank == 0:  # (nobody reads the line otherwise: skip the kinetic energy)
            try:
                temperature = self.atoms.get_temperature()
            except Exception:
                temperature = 0.0
            self.log("{} {} {} {}".format(float(energy), temperature, self.covlog, meta))
        self.step += 1
        self.results["free_energy"] = self.results["energy"]  # active.py:527
        timings.append(time.time())
        if self.report_timings:
            d = np.diff(timings)
            self.log(("timings:" + len(d) * " {:0.2g}").format(*d) + f" total: {d.sum():0.2g}")

    # ------------------------------------------------------------------ MD with the state in device memory
    def md_on_device_ok(self):
        """The device loop replaces calculate() only where calculate() does nothing the device cannot see: a
        single process, no periodic test, no force veto, one bead, and no meta-dynamics hook other than a meta.Meta over the
        built-in collective variables (device_spec(): run_md attaches it to the loop, SGPRModel.md_meta)."""
        eng = self.engine
        world = self._dist()[1]
        # (several ranks: only over the library's own exchange — every rank then integrates all atoms from the summed
        # forces and halts at the same step, sgpr_md_run)
        return (hasattr(eng, "md_run") and (world == 1 or getattr(eng, "peer_world", 1) == world) and not self.test
                and (self.meta is None or self._meta_spec() is not None) and "forces" not in self._veto and self.nbeads == 1 and eng.m > 0 and eng.mu is not None)

    def _meta_spec(self):
        """The components of self.meta as the device loop takes them, or None (no meta, a plain callable, a colvar that is not
        built in)."""
        spec = getattr(self.meta, "device_spec", None)
        return spec() if spec is not None and hasattr(self.engine, "md_meta") else None

    def _md_attach(self, eng):
        """Hook of run_md, called right after eng.md_begin(...): whatever else the device loop must evaluate beside the live
        model is attached to the run here, and the keys of what was attached are returned.  Nothing for a single model;
        BCMActiveCalculator attaches the engines of its ready members (SGPRModel.md_committee)."""
        return ()

    def _md_attached_done(self, eng, keys):
        """... and what the calculator keeps of such a run when it is over (BCMActiveCalculator: bcm_weights)."""

    def _md_gate(self, numbers):
        """The smallest covloss at which calculate() would do more than log (update_lce, active.py:806-839): below
        ediff_lb nothing happens unless a species of the frame has fewer than two inducing LCEs."""
        if not self.active:
            return 0.0  # evaluate only: never halt
        if any(self.model.indu_counts[int(z)] < 2 for z in set(int(z) for z in numbers)):
            return EPS
        return float(min(self._ediff_lb.values))

    @staticmethod
    def constraint_mask(atoms):
        """atoms.constraints as the held-component mask of the device loops ([N, 3] booleans, True = held; None without
        constraints).  Derived from what the constraints DO — each one's adjust_forces on an array of ones, the zeros it leaves —,
        not from their attributes (FixCartesian's stored mask changed its meaning between ASE versions).  Only
        ase.constraints.FixAtoms and FixCartesian (by class name: ASE's, or ase_shim's) hold Cartesian components of single
        atoms; any other kind couples atoms or directions and raises NotImplementedError."""
        cons = list(getattr(atoms, "constraints", None) or ())
        if not cons:
            return None
        ones = np.ones((len(atoms), 3))
        for c in cons:
            if type(c).__name__ not in ("FixAtoms", "FixCartesian"):
                raise NotImplementedError(f"run_md / run_relax hold atoms and Cartesian components (FixAtoms, FixCartesian); with a "
                                          f"{type(c).__name__} in atoms.constraints, drive calculate() from an ase.md / ase.optimize "
                                          f"object as theforce/cl/md.py and cl/relax.py do")
            c.adjust_forces(atoms, ones)
        return ones == 0.0

    RECORD_BYTES = 256 << 20   # the frame record of one md_run call (run_md, run_relax) stays within this much device memory

    def run_md(self, atoms, steps, temperature_K, dt_fs=1.0, friction=1e-3, rng=None, chunk=256, seed=1, sync_every=None,
               tdamp_fs=None, pfactor=None, externalstress=0.0, mask=None, iso=False, record=True, ml_filter=None, msd=None, rdf=None,
               vacf=None, vanhove=None, adf=None, sq=None):
        """`steps` steps of Langevin NVT (friction = 0: NVE) from atoms.positions / velocities, as cl/md.py:117-128 sets
        it up around this calculator — but the state stays in device memory between model updates: the integrator runs
        inside the step's last kernel (SGPRModel.md_run), the host reads 16 scalars per step and writes the same log
        line calculate() would ("energy temperature covloss", active.py:518-523), and a step whose largest covloss
        reaches the sampling threshold stops the device, is handed to calculate() — which updates the model exactly as
        it does inside an ASE loop — and the run goes on from there with the new model.  Yields (step, energy,
        temperature, updated, wall seconds) per step (device steps share the wall time of their batch evenly).  rng: a
        numpy Generator whose normal deviates move the atoms (the stream of workloads.langevin_nvt: the two loops then
        agree bit for bit), or None — the integrator draws its own on the device (counter-based on `seed`: no host
        generator and no upload on the step's path, same trajectory however the run is batched).  sync_every: steps
        k = 0 mod sync_every end a batch and atoms.positions / velocities are theirs when they are yielded (a trajectory
        writer's loginterval, cl/md.py:24); atoms.positions / velocities are current at every yield that follows an update
        and at the end.  Falls back to the host loop (workloads.langevin_nvt) where md_on_device_ok() says no.
        record (with sync_every, the device loop on one rank): the device copies the configuration of every step
        k = 0 mod sync_every into a frame record behind its evaluation (SGPRModel.md_record) and batches are NOT cut at those
        steps: the frames of a batch are fetched behind its single wait, and atoms.positions / velocities (the cell under NPT)
        are set from step k's frame before step k is yielded — what a caller observes at those yields, after updates and at
        the end is what the cutting path shows, but the loop keeps its look-ahead, its chained calls and its growing batch
        (with the reference's default loginterval = 1 the cutting path is one md_run call per step).  A batch's record stays
        within RECORD_BYTES.  record=False, and sharded runs by themselves: batches end at every multiple of sync_every.
        tdamp_fs: Nose-Hoover NVT with that damping time instead of Langevin — the reference's DEFAULT dynamics,
        md(dynamics="NPT", bulk_modulus=None) = ase.md.npt.NPT(pfactor=None, ttime=tdamp fs) (cl/md.py:17, :131-166); no
        deviates, `friction` / `rng` / `seed` unused; host loop: workloads.nose_hoover_nvt.
        pfactor (with tdamp_fs): ... and a barostat — ase.md.npt.NPT with that pfactor (ptime^2 x bulk modulus; eV, Angstrom, amu
        units as npt.NPT), externalstress (a pressure or six Voigt components), mask, iso (set_fraction_traceless(0)): the
        moving cell of cl/md.py:131-166 inside the device loop (SGPRModel.md_begin).  atoms.cell is set wherever
        atoms.positions are — sync points, a halted configuration before its calculate(), the end —, to the cell of THAT
        configuration.  The cell must be upper triangular (npt.make_cell_upper_triangular).  Host loop:
        workloads.npt_moving_cell.
        atoms.constraints: FixAtoms and FixCartesian are honoured inside the loop (constraint_mask -> SGPRModel.md_begin(fixed=);
        host loops: the twins' fixed=): the integrator sees F = 0 on a held component — self.results["forces"] stay the model's
        own, zeroing them is atoms.get_forces()' business —, its velocity is exactly 0 (the caller's value is dropped, as
        set_momenta does), it receives no noise and keeps its coordinate bit for bit.  Temperatures (the log line, the yield) are
        over the g = 3N - n_fixed remaining degrees of freedom, as atoms.get_temperature(); Nose-Hoover uses
        tfact = 2 / (g kT ttime^2) and K0 = g kT / 2, the project's own definition (ase.md.npt.NPT takes no constraints).  Not
        with a barostat; any other constraint kind: NotImplementedError.
        ml_filter: the reference's FilterDeltas around the atoms (cl/md.py:76-79, calculator/active.py:47-76) inside the loop: a
        shrink factor (0 < s < 1), or a workloads.FilterState (shrink, f, s) whose accumulators are read at the start and
        filled at the end — one holder carries them through several run_md calls, as the reference's one wrapper does.  The
        jump self.deltas that an update's calculate() publishes is pushed into the device's accumulators (SGPRModel.
        md_filter_push) before the halted configuration is evaluated again; the integrator sees the filtered forces (and, with a
        barostat, stress), self.results and the log stay the model's.  Host loops: the twins' ml_filter=.  With a filter the
        device loop runs on one rank and without a committee.  None: no filter, today's run.
        self.meta: a meta.Meta over the built-in collective variables (device_spec()) is attached to the loop behind md_begin
        (SGPRModel.md_meta: the hills it holds stand from the start, room for every deposit of the run); after every batch the
        new hill rows are appended to meta.hist and mirrored into the Meta — calculate() at a halt adds the same bias — and
        `meta: V` goes on the log lines — with pace > 1 on the lines of the depositing configurations only: the device keeps V
        per hill row, and a run goes on from a Meta only at a multiple of its pace (ValueError otherwise).  With a barostat, a committee or several ranks, and for any other meta, the host loops
        around calculate(), which adds a Meta's bias itself; there meta.update() runs once per configuration.
        A committee with members (BCMActiveCalculator) and a barostat: the device loop integrates and gates the committee in the
        moving cell (SGPRModel.md_committee on a run begun with pfactor=); such a run records no frames, so its batches end at the
        multiples of sync_every, where atoms.cell is set with atoms.positions.
        msd: a transport.Msd(every, levels, com) holder — the mean-square displacements of the run's configurations 0 ... steps
        are added to it at the end (transport.diffusion_constants reads it; one holder carries several runs).  The device loop
        accumulates them itself (SGPRModel.md_msd: two small launches behind a sampled evaluation, the table read once at the
        end); with a barostat, a committee or several ranks, and in the host loops, workloads.MsdBlocks — the same operations
        in the same order — is fed the positions of every step.  None: nothing is accumulated, today's run.
        rdf: a transport.Rdf(every, rmax, bins, rmin) holder — the pair-distance counts of the run's configurations 0 ... steps
        are added to it at the end (transport.radial_distribution forms g(r); one holder carries several runs), by the same
        conventions: the device loop counts them itself (SGPRModel.md_rdf: a pair sweep behind a sampled evaluation, the table
        read once at the end); with a committee or several ranks, and in the host loops, workloads.RdfCounts — the same integers —
        is fed the positions of every step.  The cell is constant: with a barostat NotImplementedError.
        vacf: a transport.Vacf(every, lags, origin_every, com) holder — the velocity correlations of the run's configurations
        0 ... steps are added to it at the end (transport.green_kubo, onsager and vibrational_dos read it), by the same
        conventions: the device loop accumulates them itself (SGPRModel.md_vacf: a store and a correlation behind a sampled
        evaluation, the table read once at the end); with a barostat, a committee, several ranks, ml_filter= or a Meta, and in
        the host loops, workloads.VacfRing — the same operations in the same order — is fed the velocities of every step.  The
        last sample of a run stays pending (it counts when a later one arrives), in both.
        vanhove: a transport.VanHove(every, levels, rmax, rbins, tbins, pbins, dmax, dbins) holder — the displacement histograms
        per lag and species, and with dbins > 0 the origin-to-present pair histograms, of the run's configurations 0 ... steps are
        added to it at the end (transport.displacement_histogram, self_van_hove, distinct_van_hove and non_gaussian read it), by
        the same conventions: the device loop counts them itself (SGPRModel.md_vanhove: at most three launches behind a sampled
        evaluation, the tables read once at the end); with a committee or several ranks, and in the host loops,
        workloads.VanHoveCounts — the same integers — is fed the positions of every step.  The cell is constant: with a barostat
        NotImplementedError.
        adf: a transport.Adf(every, bins, cutoffs) holder — the bond-angle counts per (centre, end, end) of species and the
        coordination counts of the run's configurations 0 ... steps are added to it at the end (transport.angle_distribution and
        coordination read it), by the same conventions: the device loop counts them itself from the step's neighbour list
        (SGPRModel.md_adf: two launches behind a sampled evaluation, the tables read once at the end; every cutoff at most the
        model's); with a committee or several ranks, and in the host loops, workloads.AdfCounts — the same integers — is fed the
        positions of every step.  The cell is constant: with a barostat NotImplementedError.
        sq: a transport.Sq(every, hkl, lags, origin_every) holder — the partial structure factors and coherent intermediate
        scattering functions of the run's configurations 0 ... steps at the wave vectors `hkl` of the cell's reciprocal lattice
        (transport.q_vectors) are added to it at the end (transport.structure_factor, intermediate_scattering and
        dynamic_structure_factor read it), by the same conventions: the device loop accumulates them itself (SGPRModel.md_sq:
        three launches behind a sampled evaluation, the tables read once at the end); with a committee or several ranks, and in
        the host loops, workloads.SqRing — the same definition, equal within md_sq.inc's bound — is fed the positions of every
        step.  The cell is constant: with a barostat NotImplementedError."""
        from .ase_shim import kB
        from .workloads import FS, MASS, FilterState, langevin_nvt, nose_hoover_nvt, npt_moving_cell
        flt = ml_filter if (ml_filter is None or hasattr(ml_filter, "shrink")) else FilterState(float(ml_filter))
        filt = {} if flt is None else dict(ml_filter=flt.shrink, filter_init=(flt.f, flt.s))
        nh = tdamp_fs is not None
        npt = pfactor is not None
        if npt and not nh:
            raise ValueError("run_md: a barostat (pfactor) needs the Nose-Hoover thermostat (tdamp_fs)")
        # the holders given, by keyword, driven through the face they share (transport._InLoop)
        holders = {k: a for k, a in dict(msd=msd, rdf=rdf, vacf=vacf, vanhove=vanhove, adf=adf, sq=sq).items() if a is not None}
        for k, a in holders.items():
            if npt and a.constant_cell:
                raise NotImplementedError(f"run_md: {k}= with a barostat (pfactor): {a.constant_cell} at constant cell")
        baro = dict(pfactor=pfactor, externalstress=externalstress, mask=mask, iso=iso) if npt else {}

        fx = held(self.constraint_mask(atoms))
        if fx is not None and npt:
            raise NotImplementedError("run_md: atoms.constraints with a barostat (pfactor): the moving-cell dynamics run "
                                      "unconstrained; drive calculate() from an ASE dynamics object instead")
        hold = {} if fx is None else dict(fixed=fx)
        numbers, pos, cell, pbc = self._system(atoms)
        N = len(numbers)
        dof = 3 * N if fx is None else 3 * N - int(fx.sum())   # (temperatures: sum m v^2 / (dof kB))
        on_device_rng = rng is None and friction > 0.0 and not nh
        rng = np.random.default_rng(seed) if rng is None else rng
        if getattr(atoms, "_masses", "ase") is None:  # (the stand-in Atoms without masses; ase.Atoms knows its own)
            masses = np.array([MASS[int(z)] for z in numbers])
            atoms._masses = masses.copy()
        else:
            masses = np.asarray(atoms.get_masses(), float)
        vel = atoms.get_velocities()
        vel = np.zeros((N, 3)) if vel is None else np.asarray(vel, float)
        if fx is not None:
            # (a held component has velocity 0 from the start, the caller's value is dropped: a first calculate() on the host
            # sees — and logs — the velocities the loops start from)
            vel = np.where(fx, 0.0, vel)
            atoms.set_velocities(vel)
        # (a committee with members — BCMActiveCalculator — runs on the device without a mask, at constant cell or under a
        # barostat (SGPRModel.md_begin(pfactor=) + md_committee: the moving cell integrates the committee's stress); with
        # constraints the host loops around calculate(), which answers with the committee, take it)
        committee = bool(getattr(self, "model_dict", None))

        def on_device():
            return (self.md_on_device_ok() and not (committee and fx is not None)
                    and not (flt is not None and (committee or self._dist()[1] > 1))
                    and not (self.meta is not None and (npt or committee or self._dist()[1] > 1))
                    and not any(a.host_only(npt, committee, self._dist()[1], flt is not None, self.meta is not None) for a in holders.values()))
        seeded = self._needs_seed() or not on_device()
        if npt:
            # (NPT.__init__ removes the mean momentum before anything is evaluated: a first calculate() on the host sees — and
            # logs — those velocities; md_begin and the host twin are handed the caller's and remove it themselves)
            from .npt import zero_mean_momentum
            atoms.set_velocities(zero_mean_momentum(vel, masses))
        if seeded:
            first_on_host(self, atoms)   # (an empty model is seeded by its first calculate(); then the device loop can take over)
            if not on_device():
                loop = (npt_moving_cell(self, numbers, pos, cell, pbc, steps, temperature_K, dt_fs, tdamp_fs, vel=vel, **baro, **filt) if npt else
                        nose_hoover_nvt(self, numbers, pos, cell, pbc, steps, temperature_K, dt_fs, tdamp_fs, vel=vel, **hold, **filt) if nh else
                        langevin_nvt(self, numbers, pos, cell, pbc, steps, temperature_K, dt_fs, friction, vel=vel, rng=rng, **hold, **filt))
                species = getattr(self.engine, "species", sorted(set(int(z) for z in numbers)))
                twins = [(a, a.twin(masses, numbers, species, cell, pbc)) for a in holders.values()]
                for st, E, T, _, p, v, *rest in loop:
                    for a, twin in twins:
                        twin.add(v if a.feeds == "velocities" else p)
                    if hasattr(self.meta, "update"):   # (the reference's dyn.attach(meta.update): calculate() has added the bias)
                        self.meta.update()
                    put_state(atoms, dict(positions=p, velocities=v, cell=rest[0] if npt else None), npt, "velocities")
                    if flt is not None:   # (the accumulators as this configuration found them: what a run that goes on from it takes)
                        flt.f, flt.s = rest[-1]
                    yield st, E, T, bool(self.updated), _
                for a, twin in twins:
                    a.add(twin.table())
                return
        eng = self.engine
        kT, dof_kB = kB * temperature_K, dof * kB
        self._peer_fit(eng, N)
        eng.md_begin(numbers, pos, cell, pbc, masses, vel, dt=dt_fs * FS, friction=0.0 if nh else friction, kT=kT,
                     seed=(int(seed) or 1) if on_device_rng else 0, ttime=tdamp_fs * FS if nh else None, **baro, **hold, **filt)
        attached = self._md_attach(eng)
        for a in holders.values():
            a.attach(eng)
        meta, meta_V = self.meta, {}
        if meta is not None:
            # the bias inside the loop: the hills the Meta holds stand from the start, room for every deposit of the run; after
            # every batch the new rows are mirrored into the Meta (meta.hist, and calculate() at a halt sees the same bias)
            meta.species = list(eng.species)   # (the twin's mean of a posvar in the device's order)
            meta.rc = float(eng.cutoff)        # (a Qlvar reads the model's list)
            if hasattr(meta, "resolve"):
                meta.resolve(np.asarray(numbers))
            if meta.pace > 1 and meta.n % meta.pace:
                # (the device counts configurations from 0 in every run: a run that goes on from a Meta in the middle of its pace
                # would deposit on another cadence than the Meta's own update())
                raise ValueError(f"run_md: the Meta has seen {meta.n} configurations, no multiple of its pace {meta.pace}: the device loop "
                                 "deposits configuration n of the run when n % pace == 0")
            hills0 = meta.hills_array()
            eng.md_meta(self._meta_spec(), meta.sigma, meta.w, tem=meta.tem, pace=meta.pace, hills=hills0 if len(hills0) else None,
                        capacity=len(hills0) + (steps + 1) // meta.pace + 2, **({"merge": meta.merge} if getattr(meta, "merge", None) else {}))
            meta_seen, meta_n0 = len(hills0), meta.n

        def hills(b):
            # the rows of the configurations below the current one (a halted one deposits when it is repeated): V by the index
            # of the configuration that deposited
            nonlocal meta_seen
            info = eng.md_meta_info()   # (the run's last configuration stands evaluated: its own row too)
            below = info["held"] if (b.final and b.code == 0) else info["below"]
            cvn, Vn = eng.md_meta_hills(meta_seen, below - meta_seen)
            first_dep = -(-b.first // meta.pace) * meta.pace
            meta.absorb(cvn, meta_n0 + b.done)
            meta_seen = below
            return {first_dep + k * meta.pace: float(v) for k, v in enumerate(Vn)}
        # (a run with members attached records no frames: batches end at the multiples of sync_every)
        rec = bool(record and sync_every and hasattr(eng, "md_record") and self._dist()[1] == 1 and not attached)
        if rec:   # (positions and the velocities the integrator holds; a batch of at most RECORD_BYTES of them)
            eng.md_record(sync_every, velocities=True, results=False)
        cap = record_cap(self.RECORD_BYTES, 48 * N, sync_every) if rec else sync_cap(sync_every) if sync_every else None
        rows = np.empty((0, N, 3))   # deviates drawn and not yet used: a halt leaves the rows behind it for the next call

        def deviates(n, final):   # (a `final` call moves nothing behind its last evaluation: one row fewer, zeros in its place)
            nonlocal rows
            need = n - 1 if final else n
            if len(rows) < need:
                rows = np.concatenate([rows, rng.normal(size=(need - len(rows), N, 3))])
            return rows[:n] if len(rows) >= n else np.concatenate([rows, np.zeros((n - len(rows), N, 3))])

        def line(t, r, prev):
            # (the line's temperature is that of the velocities the integrator holds when it asks for the forces: with a moving
            # cell the centred velocities of the configuration before, as npt.NPT hands them to calculate())
            ke = r[13] if (not npt or prev is None) else prev[12]
            return "{} {} {} {}".format(r[0], ke / dof_kB, r[11], f"meta: {meta_V[t]}" if t in meta_V else "")

        def halt(b):
            put_state(atoms, eng.md_state(results=True), npt, "velocities_pre")   # (what the integrator holds when it asks for forces)
            hand_over(self, atoms)
            if flt is not None and self.deltas:   # (the jump of this update: FilterDeltas reads it at its next call)
                eng.md_filter_push(self.deltas["forces"], self.deltas["stress"])
                flt.pushes += 1
        for b in batches(self, eng, numbers, steps, chunk, seeded, cap, None if (on_device_rng or nh) else deviates, halt):
            if meta is not None:
                meta_V = hills(b)
            counts = log_rows(self, b, line)
            out = [(t, r[0], r[12] / dof_kB, False, b.share) for t, r in enumerate(b.rows, b.first)]
            if b.resumed and out:   # (the configuration calculate() has just dealt with, evaluated again with the new model)
                out[0] = out[0][:3] + (bool(self.updated), b.share + b.t_host)
            if rec:
                # the frames of the accepted rows at multiples of sync_every, each put before its row is yielded; self.step is
                # what it is behind that row (on the cutting path a batch ends there)
                fr = recorded_frames(eng, b, sync_every)
                at = {int(i): k for k, i in enumerate(fr["index"])} if fr else {}
                for o, cnt in zip(out, counts):
                    self.step = cnt
                    if o[0] % sync_every == 0:
                        k = at[o[0]]
                        put_state(atoms, dict(positions=fr["positions"][k].copy(), velocities_pre=fr["velocities_pre"][k].copy(),
                                              cell=fr["cell"][k] if npt else None), npt, "velocities_pre")
                    yield o
            else:
                if sync_every and out and out[-1][0] % sync_every == 0 and b.code != 1:
                    # the configuration of the batch's last row: the device has moved on to the next one unless the run is over
                    put_state(atoms, eng.md_state(which=0 if b.final else -1), npt, "velocities_pre")
                yield from out
            rows = rows[len(b.rows):]
        put_state(atoms, eng.md_state(results=True), npt, "velocities")
        if flt is not None:
            flt.f, flt.s = eng.md_filter_state()
        for a in holders.values():
            a.add(a.read(eng))
        if attached:
            self._md_attached_done(eng, attached)

    def run_relax(self, atoms, fmax=0.01, steps=100000, cell=False, mask=None, clear_hist=False, chunk=256, on_frame=None, interval=1,
                  optimizer="FIRE", **fire):
        """FIRE relaxation of atoms.positions — with cell=True also of atoms.cell, through the coordinates of
        ase.constraints.UnitCellFilter(atoms, mask=mask) — as theforce/cl/relax.py minimises around this calculator, but with
        the state in device memory between model updates: run_md's loop with the optimizer in the place of the integrator
        (SGPRModel.relax_begin; md_relax.inc).  The host reads 16 scalars per evaluation and writes the log line calculate()
        would (temperature 0); an evaluation whose largest covloss reaches the sampling threshold stops the device, is handed to
        calculate() — which updates the model as inside an ASE loop —, the optimizer is re-initialised if clear_hist (and the
        model was updated), and the run goes on with the new model.  At most `steps` moves.  atoms.positions and atoms.cell are
        current after every update and at the end, where self.results are those of the final configuration.  fire: the keywords
        of ase.optimize.FIRE.  Falls back to the host loop (cl/relax.py::FIRE and UnitCellFilter around calculate()) where
        md_on_device_ok() says no, the run is sharded, or the calculator is a committee with members (the device relaxation
        evaluates one model; calculate() answers with the committee).  Returns dict(converged, steps, evaluations).
        on_frame (a trajectory writer; the optimizers' trajectory= of cl/relax.py): called as on_frame(n, dict(positions, cell,
        energy, forces)) for every accepted evaluation n that is a multiple of `interval`, and for the final structure whatever
        its index — from the frame record of the device loop (SGPRModel.md_record: the run is not cut for it; a batch's record
        stays within RECORD_BYTES), in order, behind the batch that evaluated them.  An evaluation that was handed to
        calculate() is reported once, with the results of its re-evaluation by the updated model.  The host loop calls it from
        its own steps.  Without on_frame nothing is recorded.
        atoms.constraints: FixAtoms and FixCartesian are honoured inside the loop (constraint_mask ->
        SGPRModel.relax_begin(fixed=); the host loop through the atoms' own set_positions / get_forces): the optimizer sees F = 0
        on a held component and convergence is judged on the free ones — self.results["forces"] stay the model's own —; a held
        coordinate keeps its bits at constant cell, and with cell=True keeps its undeformed coordinate while x follows the cell,
        as FixAtoms inside UnitCellFilter.  Any other constraint kind: NotImplementedError.
        optimizer = "LBFGS": L-BFGS without line search (ase/optimize/lbfgs.py; SGPRModel.relax_begin(optimizer="LBFGS"),
        md_lbfgs.inc) in the place of FIRE, `fire` then being its keywords memory, maxstep, alpha, damping; clear_hist empties
        the history through relax_reset; everything else as above.  Its host loop is workloads.lbfgs_relax — the twin of the
        device kernels — around calculate()."""
        from .cl.relax import FIRE, UnitCellFilter, force_max
        if optimizer not in ("FIRE", "LBFGS"):
            raise ValueError(f"run_relax: optimizer = 'FIRE' or 'LBFGS', not {optimizer!r}")
        fx = held(self.constraint_mask(atoms))
        hold = {} if fx is None else dict(fixed=fx)

        def device_ok():
            # (a committee with members — BCMActiveCalculator — relaxes through the host loop around calculate(): the device
            # relaxation evaluates one model)
            return (self.md_on_device_ok() and self._dist()[1] == 1 and hasattr(self.engine, "relax_begin")
                    and not getattr(self, "model_dict", None) and self.meta is None)   # (a bias: the host loop around calculate())
        seeded = self._needs_seed() or not device_ok()
        if seeded:
            first_on_host(self, atoms)
            if not device_ok():
                def report(n, last=False):
                    if on_frame is not None and (n % interval == 0 or last):
                        on_frame(n, dict(positions=np.array(atoms.positions), cell=np.array(getattr(atoms.cell, "array", atoms.cell), float),
                                         energy=float(self.results["energy"]), forces=np.array(self.results["forces"])))
                if optimizer == "LBFGS":
                    from .workloads import lbfgs_relax
                    numbers, pos, cell0, pbc = self._system(atoms)
                    o = None
                    for o in lbfgs_relax(self, numbers, pos, cell0, pbc, steps, fmax, cell_relax=cell, mask=mask,
                                         species=getattr(self.engine, "species", None), fixed=fx,
                                         reset_if=(lambda: bool(self.updated)) if clear_hist else None, **fire):
                        put_state(atoms, o, cell)
                        report(o["n"], last=o["converged"] or o["n"] == steps)
                    atoms.calc = self
                    return dict(converged=o["converged"], steps=o["n"], evaluations=o["n"] + 1)
                target = UnitCellFilter(atoms, mask=mask) if cell else atoms
                opt = FIRE(target, **fire)
                forces, n = target.get_forces(), 0
                while force_max(forces) >= fmax and n < steps:
                    report(n)
                    opt.step(forces)
                    n += 1
                    forces = target.get_forces()
                    if self.updated and clear_hist:
                        opt.initialize()
                report(n, last=True)
                return dict(converged=force_max(forces) < fmax, steps=n, evaluations=n + 1)
        numbers, pos, cell0, pbc = self._system(atoms)
        eng = self.engine
        eng.relax_begin(numbers, pos, cell0, pbc, fmax, cell_relax=cell, mask=mask, **hold, **fire, **({} if optimizer == "FIRE" else dict(optimizer=optimizer)))
        done, converged, cap = 0, False, None
        rec, reported = on_frame is not None, -1
        if rec:   # (positions and the packed results; a batch of at most RECORD_BYTES of them)
            interval = max(1, int(interval))
            eng.md_record(interval, velocities=False, results=True)
            cap = record_cap(self.RECORD_BYTES, 8 * (7 * len(numbers) + 11), interval)

        def halt(b):
            put_state(atoms, eng.md_state(), cell)
            hand_over(self, atoms)
            if clear_hist and self.updated:
                eng.relax_reset()
        for b in batches(self, eng, numbers, steps, chunk, seeded, cap, hand_over=halt):
            log_rows(self, b, lambda t, r, prev: "{} {} {} {}".format(r[0], 0.0, r[11], ""))
            fr = recorded_frames(eng, b, interval) if rec else None   # (the accepted evaluations' frames: a halted one is recorded by its re-evaluation)
            if fr:
                for k, i in enumerate(fr["index"]):
                    on_frame(int(i), dict(positions=fr["positions"][k].copy(), cell=fr["cell"][k], energy=float(fr["energy"][k]), forces=fr["forces"][k].copy()))
                    reported = int(i)
            done, converged = b.done, b.code == 3
        st = eng.md_state(results=True)
        put_state(atoms, st, cell)
        if rec and reported != done - 1:   # (the final structure, where its index is no multiple of the interval)
            on_frame(done - 1, dict(positions=st["positions"], cell=np.array(st["cell"], float), energy=float(st["energy"]), forces=st["forces"]))
        # (the calculator answers for the final configuration from what the device has just computed)
        atoms.calc = self
        Calculator.calculate(self, atoms, ("energy",), all_changes)
        self._beta = st["beta"]
        self._cov, self._nl = None, None
        self._set_results(st)
        self.results["free_energy"] = self.results["energy"]
        return dict(converged=converged, steps=max(done - 1, 0), evaluations=done)

    def run_neb(self, images, fmax=0.01, climb=False, k=0.1, steps=100000, chunk=256, on_band=None, **fire):
        """Nudged elastic band over `images` (a list of K + 2 atoms objects that share numbers, cell and pbc; the first and
        the last are the fixed ends) as theforce/cl/neb.py converges one around this calculator —
        ase.neb.NEB(images, climb=climb, allow_shared_calculator=True) under an optimizer, one calculate() per image per step —
        but with FIRE on all interior images at once and the band in device memory between model updates
        (SGPRModel.neb_begin; md_neb.inc; workloads.neb_fire is the host twin and the definition: ASE's default `aseneb`
        method, one spring constant k).  Every evaluation of the band is K plain steps of the live model; the host reads 16
        scalars per evaluation and writes one log line for it (energy of the highest image, temperature 0, largest covloss).
        An evaluation whose largest covloss over all images reaches the sampling threshold stops the device with nothing
        moved: the image that carried it gets its positions and is handed to calculate() — the on-the-fly update —; if the
        model grew, the optimizer is re-initialised (the reference's "model updated -> restart!"), and the run goes on with the
        band evaluated again by the new model.  At most `steps` moves.  Returns dict(converged, steps, evaluations, energies
        [K], forces [K, N, 3] of the interior images at the end) with the images' positions written back.
        on_band(n, state): called behind every batch with the index of its last accepted evaluation and
        SGPRModel.neb_state(results=True) of that band (positions, energy, forces [K, ...]) — a path writer.
        atoms.constraints of image 1 (FixAtoms, FixCartesian) hold the same components in every image; images whose
        constraints differ are refused.  The displacement of an atom between neighbouring images must stay well inside half a
        cell (workloads.neb_check_band).  A committee calculator is refused: the device band evaluates one model.  Where
        md_on_device_ok() says no or the run is sharded, the same loop runs on the host (neb_fire around calculate())."""
        from .workloads import neb_fire
        if hasattr(self, "model_dict"):
            raise NotImplementedError("run_neb: the band is evaluated by one model; a committee calculator (BCMActiveCalculator) "
                                      "answers with its members: drive calculate() from ase.neb.NEB as theforce/cl/neb.py does")
        images = list(images)
        K = len(images) - 2
        if K < 1:
            raise ValueError("run_neb: a band has at least one interior image between its two ends")
        masks = [self.constraint_mask(im) for im in images[1:-1]]
        fx = masks[0]
        for mk in masks[1:]:
            if (mk is None) != (fx is None) or (fx is not None and not np.array_equal(mk, fx)):
                raise NotImplementedError("run_neb: the interior images hold different components (atoms.constraints); one mask serves every image")
        fx = held(fx)
        hold = {} if fx is None else dict(fixed=fx)
        numbers, _, cell0, pbc = self._system(images[1])
        for im in images:
            n_, _, c_, p_ = self._system(im)
            if not (np.array_equal(n_, numbers) and np.array_equal(c_, cell0) and np.array_equal(p_, pbc)):
                raise ValueError("run_neb: the images of a band share numbers, cell and pbc")
        R = np.array([np.asarray(im.positions, float) for im in images])

        def device_ok():
            return self.md_on_device_ok() and self._dist()[1] == 1 and hasattr(self.engine, "neb_begin") and self.meta is None
        if self._needs_seed() or not device_ok():
            first_on_host(self, images[1])
        if not device_ok():   # the host loop: calculate() per image, a restart of the optimizer whenever the model grew
            size = [self.size]

            def grew(o):
                if self.size != size[0]:
                    size[0] = self.size
                    return "reset"
            last = None
            for last in neb_fire(self, numbers, R, cell0, pbc, steps, fmax, k=k, climb=climb, species=self.engine.species, update=grew, **hold, **fire):
                if on_band is not None:
                    on_band(last["n"], dict(positions=last["band"], energy=last["energies"], forces=last["forces"]))
            for im, x in zip(images[1:-1], last["band"]):
                im.positions = x
            return dict(converged=last["converged"], steps=last["n"], evaluations=last["n"] + 1, energies=last["energies"], forces=last["forces"])
        eng = self.engine
        eng.neb_begin(numbers, R, cell0, pbc, fmax, k=k, climb=climb, **hold, **fire)
        done, converged = 0, False

        def halt(b):   # the image that carried the largest covloss goes to calculate(), as inside an ASE loop
            i = int(b.sc[-1, 2])
            images[i].positions = eng.neb_state()["positions"][i - 1]
            size = self.size
            hand_over(self, images[i])
            if self.size != size:
                self.log("model updated -> restart!")
                eng.neb_reset()
        for b in batches(self, eng, numbers, steps, chunk, hand_over=halt):
            log_rows(self, b, lambda t, r, prev: "{} {} {} {}".format(r[0], 0.0, r[11], f"neb: highest image {int(r[1])}"))
            done, converged = b.done, b.code == 3
            if on_band is not None and b.rows:   # (the last accepted band: the current one where nothing moved behind it)
                on_band(done - 1, eng.neb_state(which=0 if (b.code == 3 or (b.code == 0 and b.final)) else -1, results=True))
        st = eng.neb_state(results=True)
        for im, x in zip(images[1:-1], st["positions"]):
            im.positions = x
        self.results = {}
        return dict(converged=converged, steps=max(done - 1, 0), evaluations=done, energies=st["energy"], forces=st["forces"])

    def _log_lines(self, lines):
        """A batch of per-step lines in one open (a device loop produces them by the hundred)."""
        if not lines:
            return
        if self.logfile and self.rank == 0:
            stamp = datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S")
            with open(self.logfile, "a") as f:
                f.write("".join("{}{} {} {}\n".format(self._logpref, stamp, st, m) for st, m in lines))
        if self.stdout and self.rank == 0:
            for _, m in lines:
                print(m)

    def veto(self):
        """active.py:537-546."""
        if self.size[0] < 2 or "forces" not in self._veto:
            return False
        if np.abs(self.results["forces"]).max() >= self._veto["forces"]:
            self.log("an update is vetoed!")
            return True
        return False

    def get_covloss(self):
        """active.py:781-804 for the last evaluated frame (computed with it on the device)."""
        return self._beta

    # ------------------------------------------------------------------ LCEs of the current frame
    def _neighbors(self):
        if self._nl is None:
            self._nl = self.engine.neighbors(len(self.atoms))
        return self._nl

    def _local_here(self, k, system=None):
        if system is None and hasattr(self.engine, "local"):
            z, r = self.engine.local(k)  # one atom's list from the device, not the whole neighbour list
            return Local(int(self.atoms.numbers[k]), z, r)
        numbers, positions, cell, _ = system or self._system(self.atoms)
        ptr, j, off = self._neighbors()
        a, b = int(ptr[k]), int(ptr[k + 1])
        r = positions[j[a:b]] - positions[k] + off[a:b].astype(float) @ cell  # descriptor/atoms.py:367-368
        return Local(int(numbers[k]), numbers[j[a:b]], r)

    def local(self, k):
        """atoms.local(k, detach=True) (descriptor/atoms.py:365-382); in a sharded run the owner of
        atom k hands the LCE to everyone."""
        rank, world = self._dist()
        if world == 1:
            return self._local_here(k)
        import torch.distributed as dist
        owner = int(rank_of_atoms(self.atoms.numbers, self.engine.species, world)[k])
        box = [self._local_here(k) if rank == owner else None]
        dist.broadcast_object_list(box, src=dist.get_global_rank(self.process_group, owner), group=self.process_group)
        return box[0]

    def _locals_of(self, numbers, positions, cell, pbc, indices=None):
        """LCEs of an arbitrary configuration (device neighbour list, unsharded)."""
        N = len(numbers)
        self.engine.predict(numbers, positions, cell, pbc, cov=False, beta=False)
        self._nl = self.engine.neighbors(N)
        sysm = (numbers, positions, cell, pbc)
        out = [self._local_here(k, sysm) for k in (range(N) if indices is None else indices)]
        self._nl = None
        return out

    # ------------------------------------------------------------------ teacher calls
    def _exact(self, atoms):
        """active.py:706-738: one teacher (ab initio) calculation."""
        tmp = atoms.copy()
        tmp.calc = self._calc
        energy = tmp.get_potential_energy()
        forces = tmp.get_forces()
        stress = tmp.get_stress()
        self.log("exact energy: {}".format(energy))
        self.log("exact stress[GPa]: {}  {}  {}".format(*(stress[:3] / GPa)))
        if self.model.ndata > 0 and "energy" in self.results:
            dE = self.results["energy"] - energy
            df = np.abs(self.results["forces"] - forces)
            self.log("predicted stress[GPa]: {}  {}  {}".format(*(self.results["stress"][:3] / GPa)))
            self.log("errors (pre):  del-E: {:.2g}  max|del-F|: {:.2g}  mean|del-F|: {:.2g}".format(
                float(dE), df.max(), df.mean()))
        self._last_test = self.step
        return energy, forces, stress

    def snapshot(self, fake=False, atoms=None):
        """active.py:740-751: the current frame with exact (teacher) or fake (own prediction) labels."""
        atoms = self.atoms if atoms is None else atoms
        if fake:
            e, f, s = self.results["energy"], self.results["forces"], self.results["stress"]
        else:
            e, f, s = self._exact(atoms)
        fr = Frame.from_atoms(atoms, e, f, s)
        if not fake and self.tape:
            self._saved_for_tape = fr
        return fr

    def head(self):
        """active.py:753-762: replace the fake labels of the newest datum by exact ones."""
        e, f, s = self._exact(self._as_atoms(self.model.data[-1]))
        self.model.refresh_targets(-1, e, f, s)
        if self.tape:
            self._saved_for_tape = self.model.data[-1]

    def _side_file(self, stem, atoms, results, mode):
        """The trajectory side files of the reference (active.py:495-499 `active_uncertain.traj`, :684-696 `active_FP.traj` /
        `active_ML.traj`): ase.io.Trajectory when ASE is installed; without it the same frames as extended XYZ (`<stem>.xyz`,
        ASE's own text format: `ase.io.read` takes it), results as energy / forces / stress of the frame.  Written beside the
        log file — the working directory for the reference's default `logfile="active.log"`, where the reference writes them —
        by calculators that keep a log: one created with `logfile=None` (a quiet evaluator inside somebody else's loop, the
        bench's timed calculate()) writes no files at all."""
        if not self.logfile:
            return
        stem = os.path.join(os.path.dirname(os.path.abspath(self.logfile)), stem)
        if HAVE_ASE:  # pragma: no cover
            import ase.io
            tmp = atoms.copy()
            tmp.calc = None if results is None else SinglePointCalculator(tmp, **results)
            ase.io.Trajectory(stem + ".traj", mode).write(tmp)
            return
        from .sgprio import Frame as XyzFrame, format_extxyz
        r = results or {}
        e = r.get("energy")
        fr = XyzFrame(np.asarray(atoms.numbers), np.asarray(atoms.positions, float), np.asarray(getattr(atoms.cell, "array", atoms.cell), float),
                      np.asarray(atoms.pbc, bool), None if e is None else float(e), r.get("forces"), r.get("stress"))
        with open(stem + ".xyz", mode) as f:
            f.writelines(format_extxyz(fr))

    def _test(self):
        """active.py:678-704."""
        energy, forces, stress = self._exact(self.atoms)
        self._ktest += 1
        if self.rank == 0:
            mode = "a" if self._ktest > 1 else "w"
            self._side_file("active_FP", self.atoms, dict(energy=energy, forces=forces, stress=stress), mode)
            self._side_file("active_ML", self.atoms, {q: self.results[q] for q in ("energy", "forces", "stress")}, mode)
        self.log("testing energy: {}".format(energy))
        dE = self.results["energy"] - energy
        df = np.abs(self.results["forces"] - forces)
        ds = np.abs(self.results["stress"] - stress)
        self.log("errors (test):  del-E: {:.2g}  max|del-F|: {:.2g}  mean|del-F|: {:.2g} mean|del-P|: {:.2g}".format(
            float(dE), df.max(), df.mean(), np.mean(ds[:3])))
        self._last_test = self.step
        return energy, forces

    # ------------------------------------------------------------------ seeding
    def initiate_model(self):
        """active.py:612-629."""
        data = [self.snapshot()]
        idx = self.get_unique_lces()
        system = self._system(self.atoms)
        inducing = self._locals_of(*system, indices=idx)
        self.model.set_data(data, inducing)
        if self.tape:
            if self._saved_for_tape is not None:
                self.tape.write(self._saved_for_tape)
                self._saved_for_tape = None
            for loc in inducing:
                self.tape.write(loc)
        details = [(int(j), int(self.atoms.numbers[j])) for j in idx]
        self.log("seed size: {} {} details: {}".format(*self.size, details))
        if self.tune_for_md:
            self.sample_rand_lces(indices=idx, repeat=1)
        self.optimize()

    def get_unique_lces(self, thresh=0.95):
        """active.py:631-654: greedy cover — atom i is kept unless k(i, j) >= thresh for a kept j.
        k(atoms, atoms) is K_mm of the frame's own LCEs, one device GEMM."""
        system = self._system(self.atoms)
        locs = self._locals_of(*system)
        scratch = self.engine.scratch()
        scratch.set_inducing(locs)
        k = scratch.M
        scratch.close()
        unique = []
        for i in range(len(locs)):
            if all(k[i, j] < thresh for j in unique):
                unique.append(i)
        return unique

    def sample_rand_lces(self, indices=None, repeat=1):
        """active.py:656-676: LCEs of a slightly rattled copy, offered to update_lce."""
        added = 0
        numbers, positions, cell, pbc = self._system(self.atoms)
        for _ in range(repeat):
            rattled = positions + np.random.uniform(-0.05, 0.05, size=positions.shape)
            order = np.random.permutation(len(numbers)) if indices is None else indices
            for loc in self._locals_of(numbers, rattled, cell, pbc, indices=order):
                added += abs(self.update_lce(loc))
        self.log(f"added {added} randomly displaced LCEs")

    # ------------------------------------------------------------------ the sampling rules
    # The sampling rules of active.py:806-984 as DATA: what to do with an environment is a function of where its covloss
    # sits relative to the two thresholds and of how many inducing LCEs its species already has.
    #   band     covloss >= ediff_ub          ediff_lb <= covloss < ediff_ub        covloss < ediff_lb
    #   m >= 2   take it (+1)                 trial against ediff                   leave it
    #   m < 2    take it, flag blind (-1)     trial against EPS (any change)        take it if covloss > EPS (-1)
    # "take" = add_inducing; "trial" = add_1inducing (add, refit, keep only if the predictions moved by the threshold).
    _TAKE, _TRIAL, _LEAVE = "take", "trial", "leave"

    def _lce_rule(self, beta, m):
        """(action, code reported when the LCE is kept, trial threshold) for a covloss and an inducing count."""
        scarce = m < 2
        if beta >= self.ediff_ub:
            return self._TAKE, (-1 if scarce else 1), None
        if beta >= self.ediff_lb:
            return self._TRIAL, None, (EPS if scarce else self.ediff)
        if scarce and beta > EPS:
            return self._TAKE, -1, None
        return self._LEAVE, 0, None

    def _covloss_of(self, loc):
        """Covloss of an environment that is not an atom of the current frame (active.py:809-818)."""
        if not (self.engine.m > 0 and self.model.choli is not None):
            return inf
        k, _ = self.engine.kernel_local(loc)
        proj = self.model.choli @ k
        with np.errstate(invalid="ignore"):
            return np.sqrt(np.maximum((1.0 - proj @ proj) * self.model._vscale.get(loc.number, inf), 0.0))

    def update_lce(self, loc, beta=None):
        """active.py:806-839: returns +1 / -1 (kept; -1: its species was short of inducing LCEs — "blind") or 0."""
        if loc.number not in self.engine.species:
            return 0
        beta = self._covloss_of(loc) if beta is None else beta
        action, code, threshold = self._lce_rule(beta, self.model.indu_counts[loc.number])
        if action == self._LEAVE:
            return 0
        if action == self._TAKE:
            self.model.add_inducing(loc)
        else:
            code, _ = self.model.add_1inducing(loc, threshold)
            if code == 0:
                return 0
        if self.model.ridge > 0.0:          # the new LCE made K_mm need a jitter: not worth having (active.py:829-831)
            self.model.pop_1inducing()
            return 0
        if self.tape:
            self.tape.write(loc)
        if self.ioptim == 0:
            self.optimize()
        return code

    def _largest_covloss(self, beta, chosen):
        """The first atom in descending order of covloss that is neither chosen nor ignored (active.py:851-856 walks
        a full argsort; only its head is ever used: one argmax over the eligible atoms, ties to the lowest index as a
        stable sort would — 0.8 ms of every step of an active run at 16384 atoms)."""
        skip = chosen + self.ignore
        if len(skip) < len(beta) and not np.isnan(beta).any():
            if not skip:
                return int(np.argmax(beta))
            masked = np.array(beta, dtype=float)
            idx = [int(i) for i in skip if 0 <= int(i) < len(masked)]   # (an `ignore` entry outside the frame is inert, as
            masked[np.asarray(idx, dtype=int)] = -inf                    # in the reference's `k not in self.ignore`)
            if np.isfinite(masked).any() or (masked == inf).any():
                return int(np.argmax(masked))
        order = np.argsort(-beta, kind="stable")
        return next((int(i) for i in order if int(i) not in chosen and int(i) not in self.ignore), int(order[-1]))

    def update_inducing(self):
        """active.py:841-885: greedy — offer the atom with the largest covloss until one is refused."""
        added_beta = added_diff = 0
        chosen = []
        added_covloss = None
        N = len(self.atoms)
        while len(chosen) < N:
            beta = self.get_covloss()
            k = self._largest_covloss(beta, chosen)
            if np.isclose(beta[k], 1.0):
                self.blind = True
            loc = self.local(k)
            added = self.update_lce(loc, beta=beta[k])
            if added == 0:
                break
            if added == -1:
                self.blind = True
                added_beta += 1
            else:
                added_diff += 1
            chosen.append(k)
            added_covloss = beta[k]
            self.update_results(covloss_only=True)  # cov gains a column, choli changed: every covloss moves
        added = added_beta + added_diff
        if added > 0:
            self.log("added indu: {} ({},{}) -> size: {} {} details: {:.2g} {}".format(
                added, added_beta, added_diff, *self.size, float(added_covloss), ""))
            if self.blind:
                self.log("model may be blind -> go robust")
        self.covlog = f"{float(np.max(self.get_covloss()))}"
        return added

    def _same_as_last_datum(self):
        """tune_for_md (active.py:888-897): the frame has barely moved since the newest datum."""
        if not (self.tune_for_md and len(self.model.data) > 2):
            return False
        last = self.model.data[-1]
        return (last.natoms == len(self.atoms) and bool((last.numbers == self.atoms.numbers).all())
                and bool((np.abs(last.positions - self.atoms.positions) < self.eps_dr).all()))

    def _optimize_after_data(self):
        """ioptim: 0 / 2 refit the hyper-parameters after every datum, k > 2 after every (k - 1)-th (active.py:919-926)."""
        if self.ioptim in (0, 2):
            self.optimize()
        elif self.ioptim > 2:
            self._ioptim = (self._ioptim + 1) % (self.ioptim - 1)
            if self._ioptim == 0:
                self.optimize()

    def update_data(self, try_fake=True, internal=False, save_model=True):
        """active.py:887-933: offer the current frame as a datum — with the model's own predictions as labels first
        (try_fake), exact ones once it is accepted.  Returns the number of data added (0 or 1)."""
        if self._same_as_last_datum():
            return 0
        before = self.model.ndata
        _, de, df = self.model.add_1atoms_fast(self.snapshot(fake=try_fake), self.ediff_tot, self.fdiff)
        added = self.model.ndata - before
        self.log(f"DF: {df}  accept: {added}")
        if added <= 0:
            return added
        if try_fake:
            self.head()
        if self.tape and self._saved_for_tape is not None:
            self.tape.write(self._saved_for_tape)
            self._saved_for_tape = None
        self.log("added data: {} -> size: {} {}".format(added, *self.size))
        self._optimize_after_data()
        if save_model:
            self.save_model()
        return added

    def optimize(self):
        self.model.make_munu(algo=3, noise_f=self.noise_f)  # active.py:939-940

    def _wants_data(self, n_lces, inducing, data):
        """Is the frame offered as a datum?  After new LCEs (if data sampling is on); and when only data are sampled
        (include_tape), whenever some covloss is still above ediff (active.py:947-951)."""
        if inducing:
            return n_lces > 0 and data
        return bool(np.max(self.get_covloss()) > self.ediff)

    def _after_model_change(self):
        """Size limits, the refit that goes with them, the three log lines, the model file (active.py:961-981)."""
        # (ioptim == 1: optimize() below refits the downsized model from the same matrix — hyper-parameter search
        # and weights — so the refit downsize would end with is the one result nobody reads)
        if any(self.model.downsize(self.max_data, self.max_inducing, first=True, lii=True, remake=self.ioptim != 1)):
            self.log("downsized -> size: {} {}".format(*self.size))
        if self.ioptim == 1:
            self.optimize()
        self.log("fit error (mean,mae): E: {:.2g} {:.2g}   F: {:.2g} {:.2g}   R2: {:.4g}".format(
            *(float(v) for v in self.model._stats)))
        self.log(f"noise: {self.model.scaled_noise}")
        self.log(f"mean: {self.model.mean}")
        self.save_model()
        self.updated = True

    def update(self, inducing=True, data=True):
        """active.py:942-984: sample LCEs, then (maybe) the frame; returns (LCEs added, data added)."""
        self.updated = self.blind = False
        n_lces = self.update_inducing() if inducing else 0
        n_data = 0
        if self._wants_data(n_lces, inducing, data):
            exact_labels = self.blind or isinstance(self._calc, SinglePointCalculator)
            n_data = self.update_data(try_fake=not exact_labels, internal=True, save_model=False)
        if n_data == 0 and data and self.step == 0 and self.step0_forced_fp:
            self.log("forced data addition")
            self.model.add_data([self.snapshot()])
            self.log("added data: {} -> size: {} {}".format(1, *self.size))
            n_data = 1
        if n_lces > 0 or n_data > 0:
            self._after_model_change()
        self._update_args = {}
        return n_lces, n_data

    def save_model(self):
        if self.pckl and self.rank == 0:
            from .modelio import save_model
            save_model(self.pckl, self.model)

    # ------------------------------------------------------------------ training from stored data
    def _as_atoms(self, fr):
        if HAVE_ASE:  # pragma: no cover
            from ase import Atoms
            return Atoms(numbers=fr.numbers, positions=fr.positions, cell=fr.cell, pbc=fr.pbc)
        from .ase_shim import Atoms
        return Atoms(fr.numbers, fr.positions, fr.cell, fr.pbc)

    def _learn_from(self, atoms, calc):
        saved = self._calc
        self._calc = calc
        try:
            atoms.calc = self
            atoms.get_potential_energy()
        finally:
            atoms.calc = calc
            self._calc = saved

    def include_data(self, data):
        """active.py:989-1004: `data` = labelled frames (Frame objects, or atoms whose .calc holds
        energy/forces/stress); each one is offered to the learner as if met during MD."""
        for item in data:
            if isinstance(item, Frame):
                atoms = self._as_atoms(item)
                calc = SinglePointCalculator(atoms, energy=item.energy, forces=item.forces, stress=item.stress)
            else:
                atoms, calc = item, item.calc
            atoms.calc = calc
            if np.abs(atoms.get_forces()).max() > self.include_params["fmax"]:
                continue
            self._learn_from(atoms, calc)

    def include_tape(self, tape, ndata=None):
        """active.py:1006-1053: replay another run's tape — its LCEs through update_lce, its frames
        through the data-acceptance test (inducing=False)."""
        if isinstance(tape, str):
            if self.tape is not None and os.path.abspath(tape) == self.tape.path:
                raise RuntimeError("ActiveCalculator can not include it own .sgpr tape!")
            tape = SgprIO(tape, rank=self.rank)
        tune_for_md, self.tune_for_md = self.tune_for_md, False
        added_lce = [0, 0]

        def _save():
            if added_lce[0] > 0:
                if self.ioptim == 1:
                    self.optimize()
                self.save_model()
                self.log("added lone indus: {}/{} -> size: {} {}".format(*added_lce, *self.size))
                self.log("fit error (mean,mae): E: {:.2g} {:.2g}   F: {:.2g} {:.2g}   R2: {:.4g}".format(
                    *(float(v) for v in self.model._stats)))

        cdata = 0
        try:
            for cls, obj in tape.read(exclude=self.tape):
                if cls == "atoms":
                    obj.check_labels()  # a frame without energy / forces cannot be learned from (stress is optional)
                    if np.abs(obj.forces).max() > self.include_params["fmax"] and len(self.model.data) > 0:
                        continue
                    _save()
                    self._update_args = dict(inducing=False)
                    atoms = self._as_atoms(obj)
                    self._learn_from(atoms, SinglePointCalculator(atoms, energy=obj.energy, forces=obj.forces,
                                                                  stress=obj.stress))
                    cdata += 1
                    if ndata and cdata >= ndata:
                        break
                    added_lce = [0, 0]
                elif cls == "local":
                    added_lce[0] += abs(self.update_lce(obj))
                    added_lce[1] += 1
            _save()
        finally:
            self.tune_for_md = tune_for_md

    def build(self):
        """active.py:1055-1098: rebuild the model from this calculator's own tape in one shot."""
        if self.pckl and os.path.exists(self.pckl):
            raise RuntimeError(f"{self.pckl} already exists and can not be overwritten by build!"
                               " remove this file and try again.")
        blocks = self.tape.read()
        data = [obj for cls, obj in blocks if cls == "atoms"]
        lce = [obj for cls, obj in blocks if cls == "local"]
        self.model.set_data(data, lce)
        self.optimize()
        self.log("built from tape {} {} -> size: {} {}".format(len(data), len(lce), *self.size))
        self.log("fit error (mean,mae): E: {:.2g} {:.2g}   F: {:.2g} {:.2g}   R2: {:.4g}".format(
            *(float(v) for v in self.model._stats)))
        self.save_model()

    # ------------------------------------------------------------------ logging (active.py:1117-1134)
    def log_settings(self):
        self.log(f"kernel: lmax={self.engine.lmax} nmax={self.engine.nmax} exponent={self.engine.exponent} "
                 f"cutoff={self.engine.cutoff} species={list(self.engine.species)}")
        self.log(f"ediff: {self._ediff}  ediff_lb: {self._ediff_lb}  ediff_ub: {self._ediff_ub}  "
                 f"ediff_tot: {self.ediff_tot}  fdiff: {self._fdiff}  noise_f: {self.noise_f}  ioptim: {self.ioptim}")

    def log(self, mssge, mode="a"):
        if self.logfile and self.rank == 0:
            with open(self.logfile, mode) as f:
                f.write("{}{} {} {}\n".format(self._logpref, datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S"),
                                              self.step, mssge))
        if self.stdout and self.rank == 0:
            print(mssge)
