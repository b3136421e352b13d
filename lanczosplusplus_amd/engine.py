"""Host-side mirror of the reference's plug-in surface for the stored-CSR Lanczos path.

`LanczosEngine` plays the roles of `InternalProductStored` (rows(), matrixVectorProduct(x, y):
x += H y; reference src/Engine/InternalProductStored.h:104-132) and of the PsimagLite
`LanczosSolver` the reference's Engine drives (computeAllStatesBelow / decomposition;
src/Engine/Engine.h:626,478).  It is a thin ctypes layer over the C ABI (include/lpp_engine.h);
all arithmetic runs in liblpp_engine.so on the GPU.  numpy arrays are the host buffers.
"""
import ctypes as C
from collections import namedtuple
from math import comb

import numpy as np

from . import _capi
from ._capi import LPP_C128, LPP_F64, Comm, Config, Stats, check


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _mat(a, L):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(L, L))


# LabeledOperator::toId (reference src/Engine/LabeledOperator.h:36-59)
OPERATORS = {"c": _capi.LPP_OP_C, "sz": _capi.LPP_OP_SZ, "cdagger": _capi.LPP_OP_CDAGGER, "n": _capi.LPP_OP_N,
             "splus": _capi.LPP_OP_SPLUS, "sminus": _capi.LPP_OP_SMINUS}
_TRANSPOSE_CONJUGATE = {"c": "cdagger", "cdagger": "c", "splus": "sminus", "sminus": "splus", "n": "n", "sz": "sz"}  # :107-119
_FERMIONIC = ("c", "cdagger")  # :100-105


def _op_id(op):
    try:
        return OPERATORS[op]
    except KeyError:
        raise ValueError("unsupported operator %r (one of %s)" % (op, ", ".join(sorted(OPERATORS))))


class LanczosEngine:
    """One engine = one GPU (one process per GPU in the multi-GPU path)."""

    def __init__(self, dtype="f64", device=0, max_steps=200, min_steps=4, eps=1e-12, reortho=False,
                 save_vectors=-1, check_lag=2, spmv_kernel=0, time_kernels=False, seed=1234, stream=None,
                 compress_values=-1):
        self._lib = _capi.lib()
        self._h = C.c_void_p()
        self.is_complex = dtype in ("c128", "complex128", np.complex128, LPP_C128)
        self.np_dtype = np.complex128 if self.is_complex else np.float64
        cfg = Config()
        self._lib.lpp_config_default(C.byref(cfg))
        cfg.device = device
        cfg.dtype = LPP_C128 if self.is_complex else LPP_F64
        cfg.max_steps = max_steps
        cfg.min_steps = min_steps
        cfg.eps = eps
        cfg.reortho = int(bool(reortho))
        cfg.save_vectors = int(save_vectors)
        cfg.check_lag = check_lag
        cfg.spmv_kernel = spmv_kernel
        cfg.time_kernels = int(bool(time_kernels))
        cfg.seed = seed
        cfg.stream = stream
        cfg.compress_values = int(compress_values)
        self.max_steps = max_steps
        self._comm_keepalive = None
        self._ctor = dict(dtype="c128" if self.is_complex else "f64", device=device, check_lag=check_lag, spmv_kernel=spmv_kernel,
                          time_kernels=time_kernels, seed=seed, compress_values=compress_values)
        self._basis = None  # (basis name, L, nup, ndown) of the model set up last, or a string: why it has no reduced density matrix
        self._model = None  # what assemble_hubbard / setup_hubbard_onthefly were given (spectral_function builds the N+-1 sectors from it)
        self._energies = None
        self._sectors = {}  # (nup, ndown) -> LanczosEngine holding that sector's Hamiltonian
        self.sector_assemblies = 0
        check(self._lib.lpp_engine_create(C.byref(self._h), C.byref(cfg)))

    def stream_ptr(self):
        """the HIP stream the engine enqueues on (lpp_engine_stream), as a ctypes void pointer"""
        return C.c_void_p(self._lib.lpp_engine_stream(self._h))

    # ---- lifetime -------------------------------------------------------------------------
    @property
    def closed(self):
        return not (getattr(self, "_h", None) is not None and self._h)

    def close(self):
        for eng in getattr(self, "_sectors", {}).values():
            eng.close()
        self._sectors = {}
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.lpp_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_solver(self, max_steps=200, min_steps=4, eps=1e-12, reortho=False, save_vectors=-1):
        """ParametersForSolver after creation (the reference builds LanczosSolver after the InternalProduct, Engine.h:608-610)."""
        check(self._lib.lpp_engine_set_solver(self._h, int(max_steps), int(min_steps), float(eps), int(bool(reortho)), int(save_vectors)))
        self.max_steps = int(max_steps)

    # ---- the stored Hamiltonian --------------------------------------------------------------
    def set_row_block(self, rows_per_block):
        """Layout hint for the next set_csr: rows_per_block = N_up of the Hubbard product basis (0 = unknown)."""
        check(self._lib.lpp_engine_set_row_block(self._h, int(rows_per_block)))

    def set_model_tj(self, L, nup, ndown, hop, jpm, jzz, w, potentialV=None):
        """describe the model behind the NEXT set_csr (lpp_engine_set_model_tj): a layout hint, verified against the CSR bit for bit"""
        hop = np.asarray(hop).reshape(L, L)
        hr = _mat(hop.real, L)
        hi = _mat(hop.imag, L) if np.iscomplexobj(hop) else None
        pv = None if potentialV is None else np.ascontiguousarray(potentialV, np.float64)
        check(self._lib.lpp_engine_set_model_tj(self._h, L, nup, ndown, _vp(hr), _vp(hi), _vp(_mat(jpm, L)), _vp(_mat(jzz, L)), _vp(_mat(w, L)),
                                                _vp(pv), 0 if pv is None else len(pv)))

    def set_model_heisenberg(self, L, szPlusConst, jpm, jzz, field=None):
        f = None if field is None else np.ascontiguousarray(field, np.float64)
        check(self._lib.lpp_engine_set_model_heisenberg(self._h, L, szPlusConst, _vp(_mat(jpm, L)), _vp(_mat(jzz, L)), _vp(f), 0 if f is None else len(f)))

    def set_csr(self, rowptr, colind, values):
        rowptr = np.ascontiguousarray(rowptr, np.int64)
        colind = np.ascontiguousarray(colind, np.int32)
        values = np.ascontiguousarray(values, self.np_dtype)
        n = len(rowptr) - 1
        if n < 0 or len(colind) != rowptr[-1] or len(values) != rowptr[-1]:
            raise ValueError("inconsistent CSR arrays")
        self._basis = None
        check(self._lib.lpp_engine_set_csr(self._h, n, _vp(rowptr), _vp(colind), _vp(values)))

    def set_csr_device(self, nrows, d_rowptr, d_colind, d_values):
        """CSR already resident on the engine's GPU: raw device addresses (e.g. torch tensor .data_ptr())."""
        self._basis = None
        check(self._lib.lpp_engine_set_csr_device(self._h, int(nrows), C.c_void_p(d_rowptr), C.c_void_p(d_colind), C.c_void_p(d_values)))

    def set_csr_partition(self, comm, global_rows, shard_starts, rowptr, colind, values):
        shard_starts = np.ascontiguousarray(shard_starts, np.int64)
        rowptr = np.ascontiguousarray(rowptr, np.int64)
        colind = np.ascontiguousarray(colind, np.int32)
        values = np.ascontiguousarray(values, self.np_dtype)
        self._comm_keepalive = comm
        self._basis = None
        check(self._lib.lpp_engine_set_csr_partition(self._h, C.byref(comm.struct), global_rows, _vp(shard_starts),
                                                     _vp(rowptr), _vp(colind), _vp(values)))

    def assemble_hubbard(self, L, nup, ndown, hop, U, V=None, comm=None, ninj=None, jcoup=None):
        """ninj: L x L Coulomb coupling of Model=HubbardOneBandExtended (the reference's second geometry term), or None;
        jcoup: L x L spin coupling (third term), with ninj Model=SuperHubbardExtended.  Model=KaneMeleHubbard: pass hop = term 0 + term 1."""
        hop = np.asarray(hop).reshape(L, L)
        hr = _mat(hop.real, L)
        hi = _mat(hop.imag, L) if np.iscomplexobj(hop) else None
        U = np.ascontiguousarray(U, np.float64)
        V = np.zeros(L) if V is None else np.ascontiguousarray(np.asarray(V, np.float64)[:L])
        nj = None if ninj is None else _mat(ninj, L)
        self._comm_keepalive = comm
        self._set_model(None if comm is not None else "assemble_hubbard", L=L, nup=nup, ndown=ndown, hop=hop, U=U, V=V, ninj=ninj, jcoup=jcoup)
        self._basis = ("hubbard", L, nup, ndown) if comm is None else None
        cs = C.byref(comm.struct) if comm is not None else None
        jc = None if jcoup is None else _mat(jcoup, L)
        check(self._lib.lpp_engine_assemble_hubbard_super(self._h, cs, L, nup, ndown, _vp(hr), _vp(hi), _vp(U), _vp(V), _vp(nj), _vp(jc)))

    def setup_hubbard_onthefly(self, L, nup, ndown, hop, U, V=None, comm=None, ninj=None, jcoup=None):
        """Matrix-free Hubbard product (InternalProductOnTheFly semantics): nothing but H_up and H_down is stored.
        jcoup (Model=SuperHubbardExtended): the spin-flip terms move both species; the product then re-derives every row from the
        term list (lpp_engine_setup_hubbard_onthefly_super)."""
        hop = np.asarray(hop).reshape(L, L)
        hr = _mat(hop.real, L)
        hi = _mat(hop.imag, L) if np.iscomplexobj(hop) else None
        U = np.ascontiguousarray(U, np.float64)
        V = np.zeros(L) if V is None else np.ascontiguousarray(np.asarray(V, np.float64)[:L])
        nj = None if ninj is None else _mat(ninj, L)
        self._comm_keepalive = comm
        self._set_model(None if comm is not None else "setup_hubbard_onthefly", L=L, nup=nup, ndown=ndown, hop=hop, U=U, V=V, ninj=ninj, jcoup=jcoup)
        self._basis = ("hubbard", L, nup, ndown) if comm is None else None
        cs = C.byref(comm.struct) if comm is not None else None
        jc = None if jcoup is None else _mat(jcoup, L)
        check(self._lib.lpp_engine_setup_hubbard_onthefly_super(self._h, cs, L, nup, ndown, _vp(hr), _vp(hi), _vp(U), _vp(V), _vp(nj), _vp(jc)))

    def assemble_heisenberg(self, L, szPlusConst, jpm, jzz, field=None, twiceS=1, anisotropy=None):
        """Heisenberg.h:80-114 on the device; twiceS > 1 or an anisotropy take the any-spin assembler (digit basis)."""
        f = None if field is None else np.ascontiguousarray(field, np.float64)
        # ReducedDensityMatrix::unpackHeisenberg reads one bit per site: S = 1/2 only
        self._basis = ("spin_half", L, szPlusConst, 0) if twiceS == 1 else "the reduced density matrix of a Heisenberg model needs twiceS = 1 (one bit per site)"
        self._set_model("assemble_heisenberg", L=L, szPlusConst=szPlusConst, jpm=jpm, jzz=jzz, field=field, twiceS=twiceS, anisotropy=anisotropy)
        if twiceS == 1 and anisotropy is None:
            check(self._lib.lpp_engine_assemble_heisenberg(self._h, L, szPlusConst, _vp(_mat(jpm, L)), _vp(_mat(jzz, L)),
                                                           _vp(f), 0 if f is None else len(f)))
            return
        a = None if anisotropy is None else np.ascontiguousarray(anisotropy, np.float64)
        check(self._lib.lpp_engine_assemble_heisenberg_spin(self._h, L, twiceS, szPlusConst, _vp(_mat(jpm, L)), _vp(_mat(jzz, L)),
                                                            _vp(f), 0 if f is None else len(f), _vp(a), 0 if a is None else len(a)))

    def assemble_tj(self, L, nup, ndown, hop, jpm, jzz, w, potentialV=None):
        hop = np.asarray(hop).reshape(L, L)
        hr = _mat(hop.real, L)
        hi = _mat(hop.imag, L) if np.iscomplexobj(hop) else None
        pv = None if potentialV is None else np.ascontiguousarray(potentialV, np.float64)
        self._basis = None  # the reference's ReducedDensityMatrix does not know this basis
        self._set_model("assemble_tj", L=L, nup=nup, ndown=ndown, hop=hop, jpm=jpm, jzz=jzz, w=w, potentialV=potentialV)
        check(self._lib.lpp_engine_assemble_tj(self._h, L, nup, ndown, _vp(hr), _vp(hi), _vp(_mat(jpm, L)),
                                               _vp(_mat(jzz, L)), _vp(_mat(w, L)), _vp(pv),
                                               0 if pv is None else len(pv)))

    def get_csr(self, which=0):
        n, nnz = C.c_int64(), C.c_int64()
        check(self._lib.lpp_engine_get_csr(self._h, which, C.byref(n), C.byref(nnz), None, None, None))
        rowptr = np.zeros(n.value + 1, np.int64)
        colind = np.zeros(nnz.value, np.int32)
        values = np.zeros(nnz.value, self.np_dtype)
        check(self._lib.lpp_engine_get_csr(self._h, which, None, None, _vp(rowptr), _vp(colind), _vp(values)))
        return rowptr, colind, values

    def rows(self):
        return self.stats()["nrows"]

    # ---- A1: x += H y -------------------------------------------------------------------------
    def matrixVectorProduct(self, x, y):
        """x += H y on host arrays (InternalProductStored::matrixVectorProduct semantics)."""
        if x.dtype != self.np_dtype or y.dtype != self.np_dtype or not x.flags.c_contiguous or not y.flags.c_contiguous:
            raise ValueError("x and y must be contiguous %s arrays" % self.np_dtype.__name__)
        n = self.rows()
        if len(x) != n or len(y) != n:
            raise ValueError("vector length %d/%d does not match rows() = %d" % (len(x), len(y), n))
        check(self._lib.lpp_engine_spmv_acc(self._h, _vp(x), _vp(y)))
        return x

    spmv_acc = matrixVectorProduct

    # ---- A2/A3: the solve ---------------------------------------------------------------------
    def _init_ptr(self, init):
        if init is None:
            return None, None
        init = np.ascontiguousarray(init, self.np_dtype)
        if len(init) != self.rows():
            raise ValueError("initial vector length does not match rows()")
        return init, _vp(init)

    def computeAllStatesBelow(self, nstates=1, init=None, want_vectors=True, init_device=None):
        """Lowest `nstates` Ritz values (and vectors): LanczosSolver::computeAllStatesBelow.
        init_device: raw device address of a start vector in the basis order on the engine's GPU (lpp_engine_lanczos_device)."""
        eigs = np.zeros(nstates, np.float64)
        zs = np.zeros((nstates, self.rows()), self.np_dtype) if want_vectors else None
        st = Stats()
        if init_device is not None:
            check(self._lib.lpp_engine_lanczos_device(self._h, C.c_void_p(int(init_device)), nstates, _vp(eigs), _vp(zs), C.byref(st)))
        else:
            keep, ip = self._init_ptr(init)
            check(self._lib.lpp_engine_lanczos(self._h, ip, nstates, _vp(eigs), _vp(zs), C.byref(st)))
        self._energies = eigs.copy()
        return eigs, zs, st.as_dict()

    lanczos = computeAllStatesBelow

    def decomposition(self, init=None, init_device=None):
        a = np.zeros(self.max_steps + 2)
        b = np.zeros(self.max_steps + 2)
        n = C.c_int32()
        st = Stats()
        if init_device is not None:
            check(self._lib.lpp_engine_decomposition_device(self._h, C.c_void_p(int(init_device)), C.byref(n), _vp(a), _vp(b), C.byref(st)))
        else:
            keep, ip = self._init_ptr(init)
            check(self._lib.lpp_engine_decomposition(self._h, ip, C.byref(n), _vp(a), _vp(b), C.byref(st)))
        return a[:n.value].copy(), b[:n.value].copy(), st.as_dict()

    # ---- incremental interface ------------------------------------------------------------------
    def begin(self, init=None, init_device=None):
        if init_device is not None:
            check(self._lib.lpp_engine_lanczos_begin_device(self._h, C.c_void_p(int(init_device))))
            return
        keep, ip = self._init_ptr(init)
        check(self._lib.lpp_engine_lanczos_begin(self._h, ip))

    def step(self, nsteps=1):
        check(self._lib.lpp_engine_lanczos_step(self._h, nsteps))

    def sync(self):
        check(self._lib.lpp_engine_sync(self._h))

    def coeffs(self):
        n = C.c_int32()
        a = np.zeros(self.max_steps + 2)
        b = np.zeros(self.max_steps + 2)
        check(self._lib.lpp_engine_lanczos_coeffs(self._h, C.byref(n), _vp(a), _vp(b)))
        return a[:n.value].copy(), b[:n.value].copy()

    def stats(self):
        st = Stats()
        check(self._lib.lpp_engine_get_stats(self._h, C.byref(st)))
        return st.as_dict()

    def layout(self, which=0):
        """HBM layout of the stored matrix (lpp_layout as a dict)."""
        lay = _capi.Layout()
        check(self._lib.lpp_engine_get_layout(self._h, which, C.byref(lay)))
        return lay.as_dict()

    def bench_spmv(self, warmup=3, iters=20):
        ms = C.c_double()
        check(self._lib.lpp_engine_bench_spmv(self._h, warmup, iters, C.byref(ms)))
        return ms.value


    # ---- observables of the four basis families of _FAMILIES (below) on one GPU -----------------------------------------
    def _set_model(self, how, **fields):
        """Record the keyword arguments of the assemble_* / setup_* method `how`, arrays copied: _sector_engine replays them on another sector.
        how=None (a partitioned engine): no model.  The sector engines of the model before are dropped."""
        self._model = None if how is None else dict(how=how, **{k: v if v is None or np.ndim(v) == 0 else np.array(v, copy=True) for k, v in fields.items()})
        for eng in self._sectors.values():
            eng.close()
        self._sectors = {}

    def _own_basis(self):
        """the name in OBS_BASES of the family the engine was set up in (assemble_heisenberg with any spin: "spin_half"); None without a model"""
        return None if self._model is None else next(b for b, f in _FAMILIES.items() if self._model["how"] in f.assemble)

    def _is_tj(self):
        return self._own_basis() == "tj"

    def _is_heis(self):
        return self._own_basis() == "spin_half"

    def _own_family(self, who, basis=None):
        """(row of _FAMILIES, sites, own sector, the two counts of the entry points) for the observables of the resident states.  basis=None: the engine's
        own family, where spins above 1/2 raise as the reference throws (BasisHeisenberg.h:130, Heisenberg.h:223).  basis="spin": the opt-in digit basis
        of a Heisenberg engine of any admitted twiceS (LPP_ERR_INVALID on any other engine).  Anything else is a ValueError."""
        m = self._need_model(who)
        own = self._own_basis()
        if basis is not None:
            if basis != "spin":
                raise ValueError("%s: unsupported basis %r (None for the engine's own, or \"spin\")" % (who, basis))
            if own != "spin_half":
                raise _capi.LppError(_capi.LPP_ERR_INVALID, "%s: basis=\"spin\" is for engines set up by assemble_heisenberg" % who)
            own = "spin"
        elif own == "spin_half":
            self._refuse_higher_spin(who)
        fam = _FAMILIES[own]
        sector = fam.sector(m)
        return fam, m["L"], sector, fam.counts(*sector, m.get("twiceS"))

    def _refuse_higher_spin(self, who):
        if self._model["twiceS"] != 1:
            raise _capi.LppError(_capi.LPP_ERR_INVALID, "%s: the observables of a Heisenberg model need twiceS = 1 (the reference throws for higher spins)" % who)

    def _destination(self, out, n, what):
        """zeros, or the caller's `out` as a contiguous vector of the engine's dtype; it must have the n elements of `what`"""
        if out is None:
            return np.zeros(n, self.np_dtype)
        z = np.ascontiguousarray(out, self.np_dtype)
        if len(z) != n:
            raise ValueError("out does not have the length of " + what)
        return z


    def keep_states_tj(self, k=1):
        """keep_states that also accepts a hole-major t-J engine (lpp_engine_keep_states_tj): state(k) is then the host Ritz vector bit for bit"""
        check(self._lib.lpp_engine_keep_states_tj(self._h, int(k)))

    def keep_states(self, k=1):
        """Keep the lowest k Ritz vectors of the next lanczos() on the device, in the basis order (lpp_engine_keep_states)."""
        check(self._lib.lpp_engine_keep_states(self._h, int(k)))

    def state_device(self, k=0):
        """(raw device address, length in elements) of resident state k"""
        p, n = C.c_void_p(), C.c_int64()
        check(self._lib.lpp_engine_state_device(self._h, int(k), C.byref(p), C.byref(n)))
        return p.value, n.value

    def state(self, k=0):
        """resident state k copied to the host"""
        _, n = self.state_device(k)
        out = np.zeros(n, self.np_dtype)
        check(self._lib.lpp_engine_state_to_host(self._h, int(k), _vp(out)))
        return out

    def apply_operator(self, op, site, spin, L, nup, ndown, src, factor=1.0, out=None, basis="hubbard", twiceS=None):
        """Engine::accModifiedState_ (Engine.h:416-458) on the GPU: returns (z, (nup', ndown')) with z[bra] += factor*sign*value*src[ket],
        z starting from `out` (new sector's length) or from zero; (None, None) where the operator leads to no sector.  src: host vector of the
        (nup, ndown) sector in the basis order.  basis: "hubbard" (BasisHubbardLanczos), "tj" (BasisTjMultiOrbLanczos, one orbital) or "spin_half"
        (BasisHeisenberg with twiceS = 1: nup = szPlusConst, ndown is not read; sz is the reference's raw 1 - 2 bit = -2 S^z, and where the reference
        throws -- c, cdagger, S+ on all ups, S- on all downs -- LppError is raised) or "spin" with twiceS=...: the digit basis of any spin
        assemble_heisenberg admits (operator_plan_heis_spin has the definition: nup = szPlusConst, ndown is not read, sz is the true S^z, n / c /
        cdagger and S+ on the top sector / S- on szPlusConst = 0 raise LppError)."""
        oid = _op_id(op)
        fam = _obs_family(basis)
        src = np.ascontiguousarray(src, self.np_dtype)
        c1, c2 = fam.counts(nup, ndown, twiceS)
        has, new, n = fam.one_site_plan(oid, site, spin, L, c1, c2)
        if not has:
            return None, None
        if len(src) != fam.size(L, c1, c2):
            raise ValueError("src does not have the length of sector (%d, %d)" % (nup, ndown))
        z = self._destination(out, n, "sector (%d, %d)" % new)
        f = complex(factor)
        call = fam.entry("lpp_engine_apply_operator", host=True)
        check(call(self._h, oid, site, spin, L, c1, c2, f.real, f.imag, _vp(src), _vp(z), int(out is not None), C.byref(C.c_int32())))
        return z, new

    def bench_operator(self, op, site, spin, L, nup, ndown, warmup=2, iters=10, basis="hubbard", twiceS=None):
        """(ms per launch, bytes of the byte model) of the operator kernel on resident vectors"""
        ms, by = C.c_double(), C.c_double()
        fam = _obs_family(basis)
        c1, c2 = fam.counts(nup, ndown, twiceS)
        check(fam.entry("lpp_engine_bench_operator")(self._h, _op_id(op), site, spin, L, c1, c2, warmup, iters, C.byref(ms), C.byref(by)))
        return ms.value, by.value

    # ---- site-weighted operator sums: |phi> = sum_r f_r A_r |src>, the modified state of A(k,w), N(q,w), S(q,w) ----
    def apply_operator_sum(self, op, spin, weights, L, nup, ndown, src, out=None, basis="hubbard", twiceS=None):
        """z (+)= sum_r weights[r] * A_r src on the GPU (lpp_engine_apply_operator_sum): returns (z, (nup', ndown')), z starting from `out` or from zero;
        (None, None) where the operator leads to no sector.  A_r is what two_point applies: c, cdagger, n of `spin`, splus, sminus as apply_operator;
        sz = n_up/2 - n_down/2 in the "hubbard" and "tj" bases, the raw 1 - 2 bit in "spin_half".  Hubbard c, cdagger, n, sz and the "spin_half" sz are ONE launch; the "tj"
        basis, splus / sminus and the "spin_half" n chain the one-site launches over the sites whose weight is not exactly 0 (as everything does under
        LPP_OBS_SUM_CHAIN=1), and so does everything in the "spin" basis (twiceS=...: sz is the true S^z).  Complex weights need a c128 engine."""
        oid = _op_id(op)
        fam = _obs_family(basis)
        c1, c2 = fam.counts(nup, ndown, twiceS)
        w = np.asarray(weights, np.complex128).ravel()
        wr, wi = np.ascontiguousarray(w.real), np.ascontiguousarray(w.imag)
        src = np.ascontiguousarray(src, self.np_dtype)
        has, n = C.c_int32(), C.c_int64()
        call = fam.entry("lpp_engine_apply_operator_sum", host=True)
        head = (self._h, oid, int(spin), int(L), c1, c2, len(w), _vp(wr), _vp(wi))
        check(call(*head, None, None, 0, C.byref(has), C.byref(n)))
        if not has.value:
            return None, None
        if len(src) != fam.size(L, c1, c2):
            raise ValueError("src does not have the length of sector (%d, %d)" % (nup, ndown))
        z = self._destination(out, n.value, "the operator's sector")
        check(call(*head, _vp(src), _vp(z), int(out is not None), C.byref(has), C.byref(n)))
        own = fam.reported(nup, ndown)
        return z, (new_parts(op, spin, L, *own, basis, twiceS) if op in ("c", "cdagger", "splus", "sminus") else own)

    def bench_operator_sum(self, op, spin, weights, L, nup, ndown, warmup=2, iters=10, accumulate=False, basis="hubbard", twiceS=None):
        """(ms per sum, bytes of the byte model: destination written -- and read when accumulating -- plus every source element once) on zeroed vectors"""
        fam = _obs_family(basis)
        w = np.asarray(weights, np.complex128).ravel()
        wr, wi = np.ascontiguousarray(w.real), np.ascontiguousarray(w.imag)
        ms, by = C.c_double(), C.c_double()
        c1, c2 = fam.counts(nup, ndown, twiceS)
        check(fam.entry("lpp_engine_bench_operator_sum")(self._h, _op_id(op), int(spin), int(L), c1, c2, len(w), _vp(wr), _vp(wi), int(bool(accumulate)), warmup, iters,
                                                         C.byref(ms), C.byref(by)))
        return ms.value, by.value

    def weighted_norm2(self, op, weights, spin=0, state=0, basis=None):
        """<phi|phi> of |phi> = sum_r weights[r] * A_r |resident state> (lpp_engine_sum_norm2): the static structure factor at the momentum the weights
        encode; 0.0 where the operator leads to no sector.  No sector engine is needed.  On an f64 engine complex weights are split as in
        spectral_function_weighted: <phi|phi> = <C|C> + <S|S>.  basis="spin": as two_point."""
        fam, L, _, (c1, c2) = self._own_family("weighted_norm2", basis)
        call = fam.entry("lpp_engine_sum_norm2")
        total = 0.0
        for _, wr, wi in self._weight_parts(weights, L):
            v, has = C.c_double(), C.c_int32()
            check(call(self._h, int(state), _op_id(op), int(spin), L, c1, c2, len(wr), _vp(wr), _vp(wi), C.byref(v), C.byref(has)))
            total += v.value
        return total

    def _weight_parts(self, weights, L):
        """[(part, w_re, w_im)]: the weights as the engine takes them.  A c128 engine, or real weights: one entry, part None.  An f64 engine with complex
        weights: the real and the imaginary weights as two REAL weight vectors, part "re" / "im"; a part whose weights are all zero is skipped."""
        w = np.asarray(weights, np.complex128).ravel()
        if len(w) != L:
            raise ValueError("one weight per site (%d), got %d" % (L, len(w)))
        wr, wi = np.ascontiguousarray(w.real), np.ascontiguousarray(w.imag)
        if self.is_complex or not np.any(wi):
            return [(None, wr, wi)]
        zero = np.zeros(L)
        return [(p, x, zero) for p, x in (("re", wr), ("im", wi)) if np.any(x)]

    def spectral_function_weighted(self, op, weights, spin=0, state=0, energy=None, max_steps=200, min_steps=4, eps=1e-12, reortho=False, basis=None):
        """The continued fractions of <phi| (z -+ (H - Eg))^-1 |phi> with |phi> = sum_r weights[r] * A_r |gs> built in one pass: the momentum-resolved
        A(k,w) (op "c" / "cdagger"), N(q,w) ("n"), S^zz(q,w) ("sz") and S(q,w) of the Heisenberg chain.  This is the project's own definition (the
        reference accumulates such a sum with a phase that does not depend on the site).  Records follow spectral_function's diagonal types: type 0 is
        the transpose-conjugate operator with CONJUGATED weights, type 1 the operator with the given weights; weight = s2 <phi|phi> with s = +1 (type 0)
        / -1 (type 1), s2 = s for a bosonic operator and 1 for c / cdagger; sigma = -s.  The state is built once: there is no doubling.  A type whose
        sector does not exist is skipped.  n and sz stay in the sector (all three bases) and NO elastic line is subtracted: the ground state's own
        contribution |<gs|phi>|^2 at w = 0 is part of the result.
        On an f64 engine complex weights are split: |phi> = C + i S with C = sum Re(f_r) A_r gs and S = sum Im(f_r) A_r gs; H is real symmetric and gs
        real, so <phi|G(z)|phi> = G_CC + G_SS, and a type gives one record per non-zero part, marked part="re" / "im".  The spectral function of a type
        is the SUM of its records' continued_fraction.  On a c128 engine, or for real weights, a type is one record with part=None.  A state of
        zero norm (sz at q = 0 in a sector with N_up = N_down) gives a record with weight 0 and no steps; continued_fraction returns 0 for it.
        basis="spin": as two_point; sz is then the true S^z, so S^zz(q,w) comes without the factor 1/4 of the S = 1/2 family's raw sz."""
        F = _, L, _, counts = self._own_family("spectral_function_weighted", basis)
        _op_id(op)
        energy = self._ground_energy("spectral_function_weighted", energy)
        if self._is_tj() and op in ("splus", "sminus") and spin != _capi.LPP_SPIN_UP:  # before any sector engine is assembled
            raise _capi.LppError(_capi.LPP_ERR_INVALID, "spectral_function_weighted: splus / sminus of the t-J basis take spin UP")
        w = np.asarray(weights, np.complex128).ravel()
        solver = dict(max_steps=max_steps, min_steps=min_steps, eps=eps, reortho=reortho, save_vectors=0)
        records = []
        for typ in (0, 1):
            o = op if typ else _TRANSPOSE_CONJUGATE[op]
            s = -1 if typ else 1

            def runs():
                return [(dict(type=typ, part=part, label="%d,%d,0,0" % (spin, typ) + ("," + part if part else "")), (int(spin), L, *counts, L, wr, wi))
                        for part, wr, wi in self._weight_parts(w if typ else np.conj(w), L)]
            records += self._spectral_type(F, "lpp_engine_spectral_decomposition_sum", o, spin, o in ("n", "sz"), state, energy, solver, s,
                                           1.0 if o in _FERMIONIC else float(s), runs)
        return records

    def _ground_energy(self, who, energy):
        if energy is None:
            if self._energies is None:
                raise _capi.LppError(_capi.LPP_ERR_STATE, "%s: run lanczos() first (after keep_states) or pass energy" % who)
            energy = float(self._energies[0])
        return energy

    def _spectral_type(self, F, stem, o, spin, stays, state, energy, solver, s, s2, runs):
        """The records of one type of spectral_function / spectral_function_weighted: operator o on resident state `state`, F from _own_family.  The
        sector is the operator's new one (none: no records) or, where it `stays`, the state's own, which gets an engine of its own (self keeps its solver
        parameters).  runs() -> [(the record's first keys, the arguments of the decomposition call `stem` between the operator and its outputs)]: one
        decomposition on the sector's engine each.  weight = s2 <modif|modif>, sigma = -s (calcSpectral, Engine.h:481-489)."""
        fam, L, own, (k1, k2) = F
        oid = OPERATORS[o]
        has, c1, c2 = C.c_int32(1), C.c_int32(own[0]), C.c_int32(own[1])
        if not stays:
            check(fam.entry("lpp_obs_new_parts")(oid, spin, L, k1, k2, C.byref(has), C.byref(c1), C.byref(c2)))
        if not has.value:
            return []
        sector, records = (c1.value, c2.value), []
        for head, args in runs():
            eng = self._sector_engine(*sector, solver)
            a = np.zeros(solver["max_steps"] + 2)
            b = np.zeros(solver["max_steps"] + 2)
            n, w, st = C.c_int32(), C.c_double(), Stats()
            check(fam.entry(stem)(self._h, int(state), eng._h, oid, *(_vp(x) if isinstance(x, np.ndarray) else x for x in args), C.byref(w), C.byref(n), _vp(a), _vp(b),
                                  C.byref(st)))
            records.append(dict(head, a=a[:n.value].copy(), b=b[:n.value].copy(), Eg=energy, weight=w.value * s2, sigma=float(-s), modif_norm2=w.value, steps=n.value,
                                sector=sector, ms_per_step=1e3 * st.seconds_total / max(st.steps_enqueued, 1), assemblies=self.sector_assemblies))
        return records

    def spectral_function_k(self, op, q, positions, **kwargs):
        """spectral_function_weighted with the momentum weights exp(i q.x_r) / sqrt(L) (geometry.momentum_weights): A(k,w), N(q,w), S(q,w)"""
        from . import geometry
        return self.spectral_function_weighted(op, geometry.momentum_weights(positions, q), **kwargs)

    # ---- products of one-site operators: -M many-point correlations and -m measure brackets (Hubbard product basis; basis="spin_half": S = 1/2 words;
    #      basis="tj": the one-orbital t-J basis) ----
    def _refuse_strings(self, who, basis="hubbard"):
        """t-J engines: LPP_ERR_INVALID naming the model unless the caller opts into the t-J basis: there sz is n of the given spin, not up minus down,
        and splus ignores its spin, so a Hubbard string carried over would silently mean something else.  Heisenberg engines likewise unless the caller
        opts into the spin basis: there sz is the raw 1 - 2 bit and n reads a spin direction."""
        fam = _string_family(basis)
        if self._is_tj() and basis != "tj":
            raise _capi.LppError(_capi.LPP_ERR_INVALID, "%s: not for the t-J (TjMultiOrb) model, operator strings are built for the Hubbard product basis; pass "
                                 "basis=\"tj\" for strings in the t-J basis (sz is then n of the given spin, the many-point convention only)" % who)
        if self._is_heis() and basis not in ("spin_half", "tj"):
            raise _capi.LppError(_capi.LPP_ERR_INVALID, "%s: not for the Heisenberg model, operator strings are built for the Hubbard product basis; pass "
                                 "basis=\"spin_half\" for strings of n, sz, splus, sminus in the spin basis (sz is then the raw 1 - 2 bit = -2 S^z)" % who)
        return fam

    def apply_operator_string(self, ops, L, nup, ndown, src, factor=1.0, out=None, convention="many_point", basis="hubbard"):
        """z (+)= factor * (the whole string applied to src) in ONE launch (lpp_engine_apply_string_host): returns (z, (nup', ndown')), z starting from `out`
        or from zero, or (None, None) where the string leads to no sector.  ops and convention as operator_string_plan.  basis="spin_half": the S = 1/2
        words of BasisHeisenberg (lpp_engine_apply_string_heis_host; ops as operator_string_plan_heis, nup = szPlusConst, ndown is not read, the
        many-point convention only); a string that is identically zero returns zeros, and LppError is raised where the reference throws.
        basis="tj": the one-orbital t-J basis (lpp_engine_apply_string_tj_host; ops as operator_string_plan_tj, the many-point convention only)."""
        fam = self._refuse_strings("apply_operator_string", basis)
        conv, off, o, s, sp, fl = _string_arrays([ops], fam.convention(convention))
        if basis == "spin_half":
            plan = operator_string_plan_heis(ops, L, nup, action=False)
            n, parts = plan["n_dst"], "%d" % plan["szPlusConst"]
        elif basis == "tj":
            plan = operator_string_plan_tj(ops, L, nup, ndown, action=False)
            if plan is None:
                return None, None
            n, parts = plan["n_dst"], "%d, %d" % (plan["nup"], plan["ndown"])
        else:
            plan = operator_string_plan(ops, L, nup, ndown, convention)
            if plan is None:
                return None, None
            n, parts = len(plan["table_up"]) * len(plan["table_down"]), "%d, %d" % (plan["nup"], plan["ndown"])
        src = np.ascontiguousarray(src, self.np_dtype)
        if len(src) != fam.size(L, nup, ndown):
            raise ValueError("src does not have the length of sector (%d, %d)" % (nup, ndown))
        z = self._destination(out, n, "sector (%s)" % parts)
        f = complex(factor)
        has, n1, n2 = C.c_int32(), C.c_int32(), C.c_int32()
        call = fam.entry("lpp_engine_apply_string", host=True)
        check(call(self._h, conv, int(off[-1]), _vp(o), _vp(s), _vp(sp), _vp(fl), L, nup, ndown, f.real, f.imag, _vp(src), _vp(z), int(out is not None), C.byref(has),
                   C.byref(n1), C.byref(n2)))
        return z, (n1.value, n2.value)

    def _brackets(self, res):
        return (res[:, 0] + 1j * res[:, 1]) if self.is_complex else res[:, 0].copy()

    def many_point(self, strings, bra=0, ket=0, convention="many_point", basis=None):
        """Engine::manyPoint (Engine.h:341-389) for a list of strings on resident states bra / ket (keep_states before lanczos): one value per string,
        conj(bra) . (O_{n-1} ... O_0 ket), the FIRST listed operator acting first.  A string is a list of (op, site, spin) or the reference's text
        "c?0?0;cdagger?1?0".  0 where a step leads to no sector (the (0,0) sector included) or the string ends in another sector; nothing is launched
        for those.  n and sz act in the sector the string has reached (the reference hands them the original sector's basis, which is ill-defined
        once the string has left it).  8 strings share one read of bra; a value does not depend on the batch it is computed in.
        basis="spin_half", on an engine set up by assemble_heisenberg with twiceS = 1 only: strings of n, sz, splus, sminus in the S = 1/2 basis
        (lpp_engine_many_point_heis; operator_string_plan_heis has the semantics: sz is the raw 1 - 2 bit = -2 S^z, n UP / DOWN is bit / 1 - bit).
        Without it a Heisenberg engine is refused.
        basis="tj", on an engine set up by assemble_tj only (keep_states_tj before lanczos; ValueError on any other engine): strings of c, cdagger, n,
        sz, splus, sminus in the one-orbital t-J basis (lpp_engine_many_point_tj; operator_string_plan_tj has the semantics: sz is n of the given
        spin, splus / sminus take spin 0).  Without it a t-J engine is refused."""
        if basis == "tj" and not self._is_tj():
            raise ValueError("many_point: basis=\"tj\" is for engines set up by assemble_tj")
        fam = self._refuse_strings("many_point", "hubbard" if basis is None else basis)
        if basis == "spin_half":
            if not self._is_heis():
                raise _capi.LppError(_capi.LPP_ERR_INVALID, "many_point: basis=\"spin_half\" is for engines set up by assemble_heisenberg (twiceS = 1)")
            self._refuse_higher_spin("many_point")
        m = self._need_model("many_point")
        conv, off, o, s, sp, fl = _string_arrays(strings, fam.convention(convention))
        res = np.zeros((len(off) - 1, 2))
        check(fam.entry("lpp_engine_many_point")(self._h, conv, len(off) - 1, _vp(off), _vp(o), _vp(s), _vp(sp), _vp(fl), m["L"], *fam.sector(m), int(bra), int(ket), _vp(res)))
        return self._brackets(res)

    def many_point_of(self, strings, L, nup, ndown, bra, ket, convention="many_point", basis="hubbard"):
        """the same for host vectors bra / ket of sector (nup, ndown) in the basis order; the engine needs no matrix.  basis="spin_half": nup = szPlusConst"""
        fam = self._refuse_strings("many_point_of", basis)
        conv, off, o, s, sp, fl = _string_arrays(strings, fam.convention(convention))
        bra = np.ascontiguousarray(bra, self.np_dtype)
        ket = np.ascontiguousarray(ket, self.np_dtype)
        if len(bra) != fam.size(L, nup, ndown) or len(ket) != len(bra):
            raise ValueError("bra / ket do not have the length of sector (%d, %d)" % (nup, ndown))
        res = np.zeros((len(off) - 1, 2))
        check(fam.entry("lpp_engine_many_point", host=True)(self._h, conv, len(off) - 1, _vp(off), _vp(o), _vp(s), _vp(sp), _vp(fl), L, nup, ndown, _vp(bra), _vp(ket), _vp(res)))
        return self._brackets(res)

    def measure(self, ops, bra=0, ket=0):
        """Engine::measure (Engine.h:208-249) through ModelBase::rahulMethod: conj(bra) . (O_0 ... O_{n-1} ket), the LAST listed operator acting first, for
        resident states.  ops: (label, site, dof, transpose) with label c / n / sz / identity, dof 0 = up, 1 = down, transpose making c into c-dagger;
        sz is -1/2 on an occupied bit of that species and +1/2 on an empty one, as RahulOperator.h has it.  A string that does not conserve both
        particle numbers raises LppError (the reference would index outside the sector)."""
        return self.many_point([ops], bra, ket, convention="measure")[0]

    def bench_string_dot(self, strings, L, nup, ndown, warmup=2, iters=10, convention="many_point", basis="hubbard"):
        """(ms per launch, bytes of the byte model) of the bracket kernel + reduction on one batch of 1 .. 8 strings, zeroed vectors"""
        fam = _string_family(basis)
        conv, off, o, s, sp, fl = _string_arrays(strings, fam.convention(convention))
        ms, by = C.c_double(), C.c_double()
        check(fam.entry("lpp_engine_bench_string_dot")(self._h, conv, len(off) - 1, _vp(off), _vp(o), _vp(s), _vp(sp), _vp(fl), L, nup, ndown, warmup, iters, C.byref(ms), C.byref(by)))
        return ms.value, by.value

    # ---- reduced density matrix of the low `split` sites (lpp_rdm.hip) ---------------------------------------
    def _rdm_call(self, call, plan, dense):
        """two calls: every refusal first (out = NULL launches nothing), then the packed result"""
        check(call(None))
        flat = np.zeros(plan["total"], self.np_dtype)
        check(call(_vp(flat)))
        blocks = [(b["k_up"], b["k_down"], b["alpha"], flat[b["offset"]:b["offset"] + b["dim"] ** 2].reshape(b["dim"], b["dim"])) for b in plan["blocks"]]
        return _rdm_dense(blocks, plan, self.np_dtype) if dense else blocks

    def reduced_density_matrix(self, split, state=0, dense=False):
        """ReducedDensityMatrix (ReducedDensityMatrix.h:65-76) of resident state `state` (keep_states before lanczos), sites 0 .. split-1 kept:
        a list of blocks (k_up, k_down, alpha, matrix), matrix[r, c] = sum over the environment of conj(psi(alpha[r], beta)) psi(alpha[c], beta)
        -- the conjugate on the row index, as the reference has it.  dense=True: the reference's square matrix of 4^split (spin 1/2: 2^split)
        rows indexed by alpha.  For engines set up by assemble_hubbard / setup_hubbard_onthefly / assemble_heisenberg with twiceS=1."""
        if self._basis is None or isinstance(self._basis, str):
            raise _capi.LppError(_capi.LPP_ERR_STATE if self._basis is None else _capi.LPP_ERR_INVALID,
                                 self._basis or "reduced_density_matrix needs an engine set up by assemble_hubbard / setup_hubbard_onthefly / assemble_heisenberg")
        basis, L, nup, ndown = self._basis
        plan = _rdm_plan_checked(L, nup, ndown, split, basis, dense)
        bid = BASES[basis]
        return self._rdm_call(lambda out: self._lib.lpp_engine_state_reduced_density_matrix(self._h, int(state), bid, L, nup, ndown, int(split), out), plan, dense)

    def reduced_density_matrix_of(self, psi, L, nup, ndown, split, basis="hubbard", dense=False):
        """the same for a host vector of sector (nup, ndown) in the basis order; the engine needs no matrix"""
        plan = _rdm_plan_checked(L, nup, ndown, split, basis, dense)
        psi = np.ascontiguousarray(psi, self.np_dtype)
        if len(psi) != plan["states"]:
            raise ValueError("psi has %d elements, the sector has %d" % (len(psi), plan["states"]))
        bid = BASES[basis]
        return self._rdm_call(lambda out: self._lib.lpp_engine_reduced_density_matrix_host(self._h, bid, L, nup, ndown, int(split), _vp(psi), out), plan, dense)

    def reduced_density_matrix_device(self, d_psi, d_out, L, nup, ndown, split, basis="hubbard"):
        """raw device addresses (16-byte aligned) on the engine's GPU: one enqueue on the engine's stream, no sync; d_out takes rdm_plan(...)["total"] elements"""
        check(self._lib.lpp_engine_reduced_density_matrix(self._h, _basis_id(basis), L, nup, ndown, int(split), C.c_void_p(int(d_psi)), C.c_void_p(int(d_out))))

    def entanglement_spectrum(self, split, state=0):
        """(eigenvalues ascending, labels): all eigenvalues of all blocks (numpy.linalg.eigvalsh per block), labels[i] = (k_up, k_down) of eigenvalue i"""
        vals, labels = [], []
        for ku, kd, _, m in self.reduced_density_matrix(split, state):
            w = np.linalg.eigvalsh(m)
            vals.append(w)
            labels += [(ku, kd)] * len(w)
        vals = np.concatenate(vals)
        order = np.argsort(vals, kind="stable")
        return vals[order], [labels[i] for i in order]

    def entanglement_entropy(self, split, state=0):
        """-sum lambda ln lambda over the eigenvalues lambda > 0 of the reduced density matrix"""
        w, _ = self.entanglement_spectrum(split, state)
        w = w[w > 0]
        return float(-np.sum(w * np.log(w)))

    def bench_rdm(self, L, nup, ndown, split, basis="hubbard", warmup=1, iters=3):
        """(ms per call, multiply-adds: sum of d^2 K over the blocks, both triangles counted, times 4 for c128) on a resident pseudo-random vector"""
        ms, macs = C.c_double(), C.c_double()
        check(self._lib.lpp_engine_bench_rdm(self._h, _basis_id(basis), L, nup, ndown, int(split), warmup, iters, C.byref(ms), C.byref(macs)))
        return ms.value, macs.value

    def _need_model(self, who):
        if self._model is None:
            raise _capi.LppError(_capi.LPP_ERR_STATE, "%s needs a single-GPU engine set up by assemble_hubbard / setup_hubbard_onthefly / assemble_tj / assemble_heisenberg" % who)
        return self._model

    def two_point(self, op, spins=(0, 0), bra=0, ket=0, basis=None):
        """Engine::twoPoint (Engine.h:266-338): (L x L matrix, trace) with result[i, j] = (A_j^{spins[1]} bra) . (A_i^{spins[0]} ket) for resident
        states bra / ket (keep_states before lanczos); -100 everywhere where the operator leads to no sector.
        basis="spin", on an engine set up by assemble_heisenberg with any admitted twiceS: the opt-in digit basis (operator_plan_heis_spin has the
        definition, the project's own: the reference throws for spins above 1/2), <S^z_j S^z_i> for "sz" and <S^-_j S^+_i> for "splus"."""
        fam, L, _, (c1, c2) = self._own_family("two_point", basis)
        res = np.zeros((L, L), self.np_dtype)
        tr = np.zeros(1, self.np_dtype)
        check(fam.entry("lpp_engine_two_point")(self._h, _op_id(op), int(spins[0]), int(spins[1]), L, c1, c2, int(bra), int(ket), _vp(res), _vp(tr)))
        return res, tr[0]

    def _sector_engine(self, nup, ndown, solver):
        eng = self._sectors.get((nup, ndown))
        if eng is None:
            eng = LanczosEngine(**self._ctor)
            replay = {k: v for k, v in self._model.items() if k != "how"}  # what the model's assemble_* / setup_* was given, on the new counts
            replay.update(zip(_FAMILIES[self._own_basis()].sector_names, (nup, ndown)))
            getattr(eng, self._model["how"])(**replay)
            self._sectors[(nup, ndown)] = eng
            self.sector_assemblies += 1
        eng.set_solver(**solver)
        return eng

    def spectral_function(self, op, isite, jsite, spin=0, state=0, energy=None, max_steps=200, min_steps=4, eps=1e-12, reortho=False, basis=None):
        """Engine::spectralFunction (Engine.h:134-206) for one (operator, site pair, spin): a list of records, one per type 0..3 (odd types: the
        operator, even types: its transpose-conjugate; a diagonal pair skips types 2 and 3; a type whose sector does not exist is skipped).
        A record is the argument list of cf.set (:489): a, b, Eg, weight (= <modif|modif> * s2), sigma (= -s), plus type, label, steps,
        ms_per_step and `assemblies` = sector Hamiltonians assembled by this engine so far (the N+-1 engines are kept, keyed by (nup, ndown)).
        max_steps .. reortho: ParametersForSolver(io, "Spectral").  energy: Eg, default the lowest eigenvalue of the last lanczos().
        basis="spin": as two_point; the sector engines are assembled with the model's twiceS and anisotropy on szPlusConst +- 1 (sz: the state's own
        sector, on a sector engine of its own)."""
        F = fam, L, _, counts = self._own_family("spectral_function", basis)
        heis = len(fam.sector_names) == 1  # (needsNewBasis() is false for n and sz, the new basis is the model's own)
        _op_id(op)
        if op in ("n", "sz") and not heis:  # before any sector engine is assembled
            raise _capi.LppError(_capi.LPP_ERR_INVALID, "spectral_function: operators that stay in the sector (n, sz) are not supported")
        energy = self._ground_energy("spectral_function", energy)
        diagonal = isite == jsite
        if self._is_tj() and op in ("splus", "sminus") and spin != _capi.LPP_SPIN_UP:  # before any sector engine is assembled
            raise _capi.LppError(_capi.LPP_ERR_INVALID, "spectral_function: splus / sminus of the t-J basis take spin UP (the reference ranks words outside the basis otherwise)")
        solver = dict(max_steps=max_steps, min_steps=min_steps, eps=eps, reortho=reortho, save_vectors=0)
        records = []
        for typ in range(2 if diagonal else 4):  # LabeledOperator::numberOfTypes; a diagonal pair has the first two
            o = op if (typ & 1) else _TRANSPOSE_CONJUGATE[op]
            s = -1 if (typ & 1) else 1
            s2 = -1.0 if typ > 1 else 1.0
            if o not in _FERMIONIC:
                s2 *= s
            s2 *= 1.0 if diagonal else 0.5
            records += self._spectral_type(F, "lpp_engine_spectral_decomposition", o, spin, heis and o in ("n", "sz"), state, energy, solver, s, s2,
                                           lambda: [(dict(type=typ, label="%d,%d,0,0" % (spin, typ)), (isite, jsite, spin, -1.0 if typ > 1 else 1.0, L, *counts))])
        return records


# ---- host-only helpers (no GPU) -------------------------------------------------------------------
OP_NAMES = tuple(OPERATORS)


# the bases ReducedDensityMatrix::unpack knows (ReducedDensityMatrix.h:78-88)
BASES = {"hubbard": _capi.LPP_BASIS_HUBBARD, "spin_half": _capi.LPP_BASIS_SPIN_HALF}
RDM_DENSE_MAX_ROWS = 4096


def _basis_id(basis):
    try:
        return BASES[basis]
    except KeyError:
        raise ValueError("unsupported basis %r (one of %s)" % (basis, ", ".join(sorted(BASES))))


def rdm_plan(L, nup, ndown, split, basis="hubbard"):
    """The plan of the reduced density matrix of sites 0 .. split-1 (lpp_rdm_plan): a dict with `blocks` (ascending (k_down, k_up); each a dict of
    k_up, k_down, dim_up, dim_down, dim, env_up, env_down, terms = env_up * env_down, offset, alpha = the alpha word of every row), `total`
    (packed elements), `states` (the sector's size) and `starts_up` / `starts_down`: {k: run-start ranks of the environment words, ascending}.
    basis "spin_half": nup = number of set bits, ndown is ignored."""
    lib = _capi.lib()
    bid = _basis_id(basis)
    nb, tot, rows, nsu, nsd = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    args = (bid, int(L), int(nup), int(ndown), int(split), C.byref(nb), C.byref(tot), C.byref(rows), C.byref(nsu), C.byref(nsd))
    check(lib.lpp_rdm_plan(*args, None, None, None, None))
    blk = (_capi.RdmBlock * nb.value)()
    alpha, su, sd = np.zeros(rows.value, np.int64), np.zeros(nsu.value, np.int64), np.zeros(nsd.value, np.int64)
    check(lib.lpp_rdm_plan(*args, C.cast(blk, C.c_void_p), _vp(alpha), _vp(su), _vp(sd)))
    if bid == _capi.LPP_BASIS_SPIN_HALF:
        ndown = 0
    blocks, r = [], 0
    for b in blk:
        d = b.dim_up * b.dim_down
        blocks.append(dict(k_up=b.k_up, k_down=b.k_down, dim_up=b.dim_up, dim_down=b.dim_down, dim=d, env_up=b.env_up, env_down=b.env_down,
                           terms=b.env_up * b.env_down, offset=b.offset, alpha=alpha[r:r + d].copy()))
        r += d

    def by_class(tab, n):
        out, o = {}, 0
        for k in range(max(0, n - (L - split)), min(split, n) + 1):
            c = comb(L - split, n - k)
            out[k] = tab[o:o + c].copy()
            o += c
        return out

    return dict(blocks=blocks, total=tot.value, states=comb(L, nup) * comb(L, ndown), starts_up=by_class(su, nup), starts_down=by_class(sd, ndown),
                dense_rows=(2 if bid == _capi.LPP_BASIS_SPIN_HALF else 4) ** split)


def _rdm_plan_checked(L, nup, ndown, split, basis, dense):
    _basis_id(basis)
    if dense and 0 <= split <= L and (2 if basis == "spin_half" else 4) ** split > RDM_DENSE_MAX_ROWS:
        raise ValueError("dense=True: the matrix would have more than %d rows; take the blocks" % RDM_DENSE_MAX_ROWS)
    return rdm_plan(L, nup, ndown, split, basis)


def _rdm_dense(blocks, plan, dtype):
    out = np.zeros((plan["dense_rows"], plan["dense_rows"]), dtype)
    for _, _, alpha, m in blocks:
        out[np.ix_(alpha, alpha)] = m
    return out


# ---- the observable families: everything above and below that depends on the basis asks one row of this table ----
class _Family(namedtuple("_Family", "name suffix counts size plan conventions sector_names assemble")):
    """name: the `basis` argument.  suffix: of the family's C entry points.  counts(nup, ndown, twiceS): the two counts those take.  size(L, *counts):
    states of the sector.  plan(lib, head, has, n1, n2, nu, nd, lb): the family's lpp_obs_plan* call without tables, head = (op, site, spin, L, *counts).
    conventions: of its operator strings, () where it has none.  sector_names: the arguments of its assemble_* that name the sector; with one name a
    sector is reported as (count, 0).  assemble: the LanczosEngine methods that make an engine of the family."""
    __slots__ = ()

    def entry(self, stem, host=False):
        """the family's C entry point of that stem, e.g. lpp_engine_apply_operator_tj_host"""
        return getattr(_capi.lib(), stem + self.suffix + ("_host" if host else ""))

    def reported(self, nup, ndown):
        return (nup, ndown) if len(self.sector_names) == 2 else (nup, 0)

    def sector(self, model):
        """the sector of a recorded model (LanczosEngine._set_model), as reported"""
        return self.reported(*(tuple(model[k] for k in self.sector_names) + (0,))[:2])

    def one_site_plan(self, op, site, spin, L, c1, c2):
        """(has, the new sector as reported, n_dst) of one operator application"""
        has, n1, n2, lb, nu, nd = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(1), C.c_int64()
        check(self.plan(_capi.lib(), (op, site, spin, L, c1, c2), *(C.byref(x) for x in (has, n1, n2, nu, nd, lb))))
        return bool(has.value), (n1.value, n2.value), nu.value * nd.value

    def convention(self, convention):
        """the convention as given; the spin and t-J bases have the many-point one only (RahulOperator's labels are per fermion species, and on the t-J
        basis it is not restated)"""
        if self.conventions == ("many_point",) and convention != "many_point":
            raise ValueError("basis=\"%s\" has convention=\"many_point\" only, not %r" % (self.name, convention))
        return convention


def _two_counts(nup, ndown, twiceS):
    return int(nup), int(ndown)


def _spin_counts(nup, ndown, twiceS):
    """(twiceS, szPlusConst = nup), and twiceS is required"""
    if twiceS is None:
        raise ValueError("basis=\"spin\" needs twiceS")
    return int(twiceS), int(nup)


def _digit_words(L, t, m):
    """the words of L digits 0 .. t whose digits add up to m"""
    count = [1] + [0] * (L * t)  # strings of no digit
    for _ in range(L):
        count = [sum(count[max(0, s - t):s + 1]) for s in range(L * t + 1)]
    return count[m] if 0 <= m <= L * t else 0


_FAMILIES = {f.name: f for f in (
    _Family(name="hubbard", suffix="", counts=_two_counts, size=lambda L, nup, ndown: comb(L, nup) * comb(L, ndown),
            plan=lambda lib, head, has, n1, n2, nu, nd, lb: lib.lpp_obs_plan(*head, has, n1, n2, nu, nd, None, None),
            conventions=("many_point", "measure"), sector_names=("nup", "ndown"), assemble=("assemble_hubbard", "setup_hubbard_onthefly")),
    _Family(name="tj", suffix="_tj", counts=_two_counts, size=lambda L, nup, ndown: comb(L, ndown) * comb(L - ndown, nup) if nup + ndown <= L else 0,
            plan=lambda lib, head, has, n1, n2, nu, nd, lb: lib.lpp_obs_plan_tj(*head, has, n1, n2, nd, None),
            conventions=("many_point",), sector_names=("nup", "ndown"), assemble=("assemble_tj",)),
    _Family(name="spin_half", suffix="_heis", counts=_two_counts, size=lambda L, nup, ndown: comb(L, nup),
            plan=lambda lib, head, has, n1, n2, nu, nd, lb: lib.lpp_obs_plan_heis(*head, has, n1, n2, nd, lb, None),
            conventions=("many_point",), sector_names=("szPlusConst",), assemble=("assemble_heisenberg",)),
    # the opt-in digit basis of a Heisenberg engine of any admitted spin (an engine's own family is the FIRST row that names its assemble method)
    _Family(name="spin", suffix="_heis_spin", counts=_spin_counts, size=_digit_words,
            plan=lambda lib, head, has, n1, n2, nu, nd, lb: lib.lpp_obs_plan_heis_spin(*head, has, n1, nd, lb, None, None),
            conventions=(), sector_names=("szPlusConst",), assemble=("assemble_heisenberg",)))}
OBS_BASES = tuple(_FAMILIES)
STRING_BASES = tuple(sorted(b for b, f in _FAMILIES.items() if f.conventions))


def _obs_family(basis):
    if basis not in OBS_BASES:
        raise ValueError("unsupported basis %r (one of %s)" % (basis, ", ".join(OBS_BASES)))
    return _FAMILIES[basis]


def _string_family(basis):
    if basis not in STRING_BASES:
        raise ValueError("unsupported basis %r for operator strings (one of %s)" % (basis, ", ".join(STRING_BASES)))
    return _FAMILIES[basis]


def sector_size(L, nup, ndown, basis="hubbard", twiceS=None):
    """states of the sector; basis="spin" (twiceS=...): the words of L digits 0 .. twiceS whose digits add up to nup = szPlusConst"""
    fam = _obs_family(basis)
    return fam.size(L, *fam.counts(nup, ndown, twiceS))

def new_parts(op, spin, L, nup, ndown, basis="hubbard", twiceS=None):
    """HubbardOneOrbital::hasNewParts (basis="tj": TjMultiOrb::hasNewParts, basis="spin_half": Heisenberg::hasNewParts with nup = szPlusConst, the new
    sector as (szPlusConst', 0)): the new (nup, ndown), or None where the reference returns false (LPP_ERR_INVALID where it throws: n, for the t-J model
    sz, for the Heisenberg model c, cdagger, S+ on all ups and S- on all downs).  basis="spin" with twiceS=...: the digit basis of any admitted spin,
    nup = szPlusConst, the new sector as (szPlusConst', 0); LPP_ERR_INVALID for n, c, cdagger, S+ on the top sector and S- on szPlusConst = 0."""
    has, n1, n2 = C.c_int32(), C.c_int32(), C.c_int32()
    fam = _obs_family(basis)
    c1, c2 = fam.counts(nup, ndown, twiceS)
    check(fam.entry("lpp_obs_new_parts")(_op_id(op), spin, L, c1, c2, C.byref(has), C.byref(n1), C.byref(n2)))
    return (n1.value, n2.value) if has.value else None


def operator_plan_tj(op, site, spin, L, nup, ndown):
    """The expanded plan of one operator application in the t-J basis (lpp_obs_plan_tj): None where the operator leads to no sector, else a dict with
    the new sector and action[dst] = +-(src + 1) or 0, expanded on the host through the tables and the lookup function the kernel uses."""
    lib = _capi.lib()
    oid = _op_id(op)
    has, n1, n2, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    check(lib.lpp_obs_plan_tj(oid, site, spin, L, nup, ndown, C.byref(has), C.byref(n1), C.byref(n2), C.byref(n), None))
    if not has.value:
        return None
    action = np.zeros(n.value, np.int64)
    check(lib.lpp_obs_plan_tj(oid, site, spin, L, nup, ndown, C.byref(has), C.byref(n1), C.byref(n2), C.byref(n), _vp(action)))
    return dict(nup=n1.value, ndown=n2.value, action=action)


def operator_plan_heis(op, site, spin, L, szPlusConst):
    """The expanded plan of one operator application in the S = 1/2 Heisenberg basis (lpp_obs_plan_heis): a dict with the new sector (nup = szPlusConst',
    ndown = 0), action[dst] = +-(src + 1) or 0, expanded on the host through the run table and the lookup function the kernel uses, and lb: the cut of
    the word (a site below it gathers inside the runs of equal high part, a site at or above it maps run onto run).  Raises where the reference throws."""
    lib = _capi.lib()
    oid = _op_id(op)
    has, n1, n2, n, lb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
    check(lib.lpp_obs_plan_heis(oid, site, spin, L, szPlusConst, 0, C.byref(has), C.byref(n1), C.byref(n2), C.byref(n), C.byref(lb), None))
    action = np.zeros(n.value, np.int64)
    check(lib.lpp_obs_plan_heis(oid, site, spin, L, szPlusConst, 0, C.byref(has), C.byref(n1), C.byref(n2), C.byref(n), C.byref(lb), _vp(action)))
    return dict(nup=n1.value, ndown=n2.value, action=action, lb=lb.value)


def operator_plan_heis_spin(op, site, L, twiceS, szPlusConst):
    """The expanded plan of one operator application in the digit basis of a spin-S Heisenberg model (lpp_obs_plan_heis_spin; the project's own
    definition, the reference throws for spins above 1/2).  Words of L digits of `bits` bits, site p at bit offset p * bits, digit d = m + S in
    [0, twiceS], digit sum szPlusConst, ascending.  With m = d - S of the source: splus d -> d + 1 with value sqrt(S(S+1) - m(m+1)), sminus d -> d - 1
    with sqrt(S(S+1) - m(m-1)), sz keeps the index with value m (a value of 0 leaves the destination untouched).  Returns a dict with the new sector
    (nup = szPlusConst', ndown = 0), action[dst] = src + 1 or 0, coef[dst] = the value, both expanded on the host through the run table and the lookup
    function the kernel uses, and lb: the cut of the word in digits.  Raises for n, c, cdagger, S+ on the top sector, S- on szPlusConst = 0 and for
    spins the assembler refuses."""
    lib = _capi.lib()
    oid = _op_id(op)
    has, m2, n, lb = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
    head = (oid, int(site), 0, int(L), int(twiceS), int(szPlusConst), C.byref(has), C.byref(m2), C.byref(n), C.byref(lb))
    check(lib.lpp_obs_plan_heis_spin(*head, None, None))
    action, coef = np.zeros(n.value, np.int64), np.zeros(n.value)
    check(lib.lpp_obs_plan_heis_spin(*head, _vp(action), _vp(coef)))
    return dict(nup=m2.value, ndown=0, action=action, coef=coef, lb=lb.value)


def operator_plan(op, site, spin, L, nup, ndown):
    """The plan of one operator application (lpp_obs_plan): None where the operator leads to no sector, else a dict with the new sector and the two
    per-species tables, table[destination species rank] = +-(source species rank + 1) or 0 (for sz: the two occupancy tables)."""
    lib = _capi.lib()
    oid = _op_id(op)
    has, n1, n2 = C.c_int32(), C.c_int32(), C.c_int32()
    nu, nd = C.c_int64(), C.c_int64()
    check(lib.lpp_obs_plan(oid, site, spin, L, nup, ndown, C.byref(has), C.byref(n1), C.byref(n2), C.byref(nu), C.byref(nd), None, None))
    if not has.value:
        return None
    tu, td = np.zeros(nu.value, np.int32), np.zeros(nd.value, np.int32)
    check(lib.lpp_obs_plan(oid, site, spin, L, nup, ndown, C.byref(has), C.byref(n1), C.byref(n2), C.byref(nu), C.byref(nd), _vp(tu), _vp(td)))
    return dict(nup=n1.value, ndown=n2.value, table_up=tu, table_down=td)


def operator_sum_plan(op, spin, L, nup, ndown, weights=None):
    """The fused plan of sum_r f_r A_r in the Hubbard product basis (lpp_obs_sum_plan), expanded on the host in the kernel's order: None where the
    operator leads to no sector, else a dict with the new sector, n_dst, width (sources per destination: L - n or n for c / cdagger, 1 for n / sz) and
    (n_dst, width) arrays src (source index), site (whose weight applies; -1 for n / sz) and factor (sign * f_site; for n / sz the element's whole
    coefficient).  weights: default all ones, so that factor is the sign.  Raises for splus / sminus (no fused plan) and where operator_plan raises."""
    lib = _capi.lib()
    oid = _op_id(op)
    w = np.ones(L, np.complex128) if weights is None else np.asarray(weights, np.complex128).ravel()
    if len(w) != L:
        raise ValueError("one weight per site (%d), got %d" % (L, len(w)))
    wr, wi = np.ascontiguousarray(w.real), np.ascontiguousarray(w.imag)
    has, n1, n2, n, wd = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
    head = (oid, int(spin), int(L), int(nup), int(ndown), _vp(wr), _vp(wi), C.byref(has), C.byref(n1), C.byref(n2), C.byref(n), C.byref(wd))
    check(lib.lpp_obs_sum_plan(*head, None, None, None, None))
    if not has.value:
        return None
    shape = (n.value, wd.value)
    src, site, fr, fi = np.zeros(shape, np.int64), np.zeros(shape, np.int32), np.zeros(shape), np.zeros(shape)
    check(lib.lpp_obs_sum_plan(*head, _vp(src), _vp(site), _vp(fr), _vp(fi)))
    return dict(nup=n1.value, ndown=n2.value, n_dst=n.value, width=wd.value, src=src, site=site, factor=fr + 1j * fi)


# RahulOperator::fromString (RahulOperator.h:56-63)
MEASURE_LABELS = {"c": _capi.LPP_OP_C, "n": _capi.LPP_OP_N, "sz": _capi.LPP_OP_SZ, "identity": _capi.LPP_OP_IDENTITY}
STRING_CONVENTIONS = {"many_point": _capi.LPP_STRING_MANY_POINT, "measure": _capi.LPP_STRING_MEASURE}


def parse_many_point(text):
    """the reference's -M text (LanczosDriver1.h:24-40): "op?site?spin[?orbital];..." -> [(op, site, spin), ...]; orbital 0 only"""
    out = []
    for tok in text.split(";"):
        parts = tok.split("?")
        if len(parts) < 3 or len(parts) > 4:
            raise ValueError("-M option malformed: %r" % tok)
        if len(parts) == 4 and int(parts[3]) != 0:
            raise ValueError("orbital 0 only: %r" % tok)
        out.append((parts[0], int(parts[1]), int(parts[2])))
    return out


def _string_arrays(strings, convention):
    """(convention id, offsets, ops, sites, spins, flags) as the C entry points take a list of strings"""
    try:
        conv = STRING_CONVENTIONS[convention]
    except KeyError:
        raise ValueError("unsupported convention %r (one of %s)" % (convention, ", ".join(sorted(STRING_CONVENTIONS))))
    off, ops, sites, spins, flags = [0], [], [], [], []
    for string in strings:
        if isinstance(string, str):
            if convention != "many_point":
                raise ValueError("text strings are the -M form; pass measure operators as (label, site, dof, transpose)")
            string = parse_many_point(string)
        for item in string:
            if convention == "measure":
                label, site, dof = item[0], item[1], item[2]
                if label not in MEASURE_LABELS:
                    raise ValueError("unsupported label %r (one of %s)" % (label, ", ".join(sorted(MEASURE_LABELS))))
                ops.append(MEASURE_LABELS[label])
                flags.append(int(bool(item[3])) if len(item) > 3 else 0)
            else:
                label, site, dof = item
                ops.append(_op_id(label))
                flags.append(0)
            sites.append(int(site))
            spins.append(int(dof))
        off.append(len(ops))
    pad = [0] if not ops else []  # (a valid pointer for an empty list)
    return (conv, np.array(off, np.int64), np.array(ops + pad, np.int32), np.array(sites + pad, np.int32), np.array(spins + pad, np.int32),
            np.array(flags + pad, np.int32))


def operator_string_plan_tj(ops, L, nup, ndown, action=True):
    """The plan of a product of c, cdagger, n, sz, splus, sminus in the one-orbital t-J basis (lpp_obs_string_plan_tj, host only), ops = (op, site, spin)
    or the -M text, the first acting first (Engine::manyPoint with BasisTjMultiOrbLanczos::getBraIndex): c / cdagger flip the species' own bit with
    doSignGf, n and a raw sz are both "the bit of the given spin is set", splus makes a down site up and sminus an up site down (spin 0; value 1, no
    sign); the sectors walk by TjMultiOrb::hasNewParts.  None where a step leads to no sector, else a dict with the final sector (nup, ndown), dead (the
    string is identically zero), the words of
        result[(u, d)] = sign * (-1)^popcount(us & par_up) * (-1)^popcount(ds & par_down) * src[index(us, ds)],  us = u ^ flip_up, ds = d ^ flip_down,
        where (us & mask) == want_up and (ds & mask) == want_down,
    n_dst, touched (the destinations the string reaches, in closed form) and, with action, action[dst] = +-(src + 1) or 0 expanded through the
    per-down-word entries and the lookup function the kernels use."""
    lib = _capi.lib()
    conv, off, o, s, sp, fl = _string_arrays([ops], "many_point")
    has, n1, n2, dead, sign = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    n, touched = C.c_int64(), C.c_int64()
    words = np.zeros(7, np.uint32)
    args = (conv, int(off[-1]), _vp(o), _vp(s), _vp(sp), _vp(fl), int(L), int(nup), int(ndown), C.byref(has), C.byref(n1), C.byref(n2), C.byref(dead), _vp(words),
            C.byref(sign), C.byref(n), C.byref(touched))
    check(lib.lpp_obs_string_plan_tj(*args, None))
    if not has.value:
        return None
    out = dict(nup=n1.value, ndown=n2.value, dead=bool(dead.value), sign=sign.value, n_dst=n.value, touched=touched.value)
    out.update(zip(("flip_up", "flip_down", "mask", "want_up", "want_down", "par_up", "par_down"), (int(w) for w in words)))
    if action:
        out["action"] = np.zeros(n.value, np.int64)
        check(lib.lpp_obs_string_plan_tj(*args, _vp(out["action"])))
    return out


def operator_string_plan_heis(ops, L, szPlusConst, action=True):
    """The plan of a product of n, sz, splus, sminus in the S = 1/2 Heisenberg basis (lpp_obs_string_plan_heis, host only), ops = (op, site, spin) or the
    -M text, the first acting first (Engine::manyPoint with BasisHeisenberg::getBraIndex): splus / sminus flip the site's bit where it is clear / set
    (value 1, the spin is not read), n is bit (spin UP) or 1 - bit (DOWN), sz is 1 - 2 bit; no sign.  A dict with the final szPlusConst, dead (the
    string is identically zero), the five words of
        result[d] = sign * (-1)^popcount((d ^ flip) & zmask) * src[rank(d ^ flip)]   where ((d ^ flip) & need) == want,
    lb (the cut of the word), n_dst and, with action, action[dst] = +-(src + 1) or 0 expanded through the run entries and the lookup function the
    kernels use.  Raises where the reference throws: c / cdagger, S+ met in the all-up sector, S- met in the all-down one."""
    lib = _capi.lib()
    conv, off, o, s, sp, fl = _string_arrays([ops], "many_point")
    m2, dead, sign, lb, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    words = [C.c_uint64() for _ in range(4)]
    args = (conv, int(off[-1]), _vp(o), _vp(s), _vp(sp), _vp(fl), int(L), int(szPlusConst), 0, C.byref(m2), C.byref(dead)) + tuple(C.byref(w) for w in words) + (
        C.byref(sign), C.byref(lb), C.byref(n))
    check(lib.lpp_obs_string_plan_heis(*args, None))
    out = dict(szPlusConst=m2.value, dead=bool(dead.value), flip=words[0].value, need=words[1].value, want=words[2].value, zmask=words[3].value, sign=sign.value,
               lb=lb.value, n_dst=n.value)
    if action:
        out["action"] = np.zeros(n.value, np.int64)
        check(lib.lpp_obs_string_plan_heis(*args, _vp(out["action"])))
    return out


def operator_string_plan(ops, L, nup, ndown, convention="many_point"):
    """The plan of a product of one-site operators (lpp_obs_string_plan, host only): None where the string leads to no sector, else a dict with the
    final sector (nup, ndown), scale, the two composed tables table[destination species rank] = +-(source species rank + 1) or 0, and sz: a list of
    (site, flip_up, flip_down) whose factors (bit_up(src, site) ^ flip_up) - (bit_down(src, site) ^ flip_down) multiply the coefficient.
    convention "many_point": ops = (op, site, spin), the first acts first (Engine::manyPoint); "measure": ops = (label, site, dof, transpose), the
    last acts first (ModelBase::rahulMethod)."""
    lib = _capi.lib()
    conv, off, o, s, sp, fl = _string_arrays([ops], convention)
    has, n1, n2, nsz = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    nu, nd, scale = C.c_int64(), C.c_int64(), C.c_double()
    args = (conv, int(off[-1]), _vp(o), _vp(s), _vp(sp), _vp(fl), int(L), int(nup), int(ndown), C.byref(has), C.byref(n1), C.byref(n2), C.byref(scale), C.byref(nu), C.byref(nd))
    check(lib.lpp_obs_string_plan(*args, None, None, C.byref(nsz), None))
    if not has.value:
        return None
    tu, td, sz = np.zeros(nu.value, np.int32), np.zeros(nd.value, np.int32), np.zeros(3 * 16, np.int32)
    check(lib.lpp_obs_string_plan(*args, _vp(tu), _vp(td), C.byref(nsz), _vp(sz)))
    return dict(nup=n1.value, ndown=n2.value, scale=scale.value, table_up=tu, table_down=td, sz=[tuple(int(v) for v in sz[3 * k:3 * k + 3]) for k in range(nsz.value)])


def continued_fraction(record, z):
    """G(z) = w / (z + sigma (a_0 - Eg) - b_0^2 / (z + sigma (a_1 - Eg) - ...)) for a record of spectral_function (or any mapping with a, b, Eg,
    weight, sigma); b_k is the decomposition's coefficient at index k, the one that couples Lanczos vectors k and k+1.  The project's own
    convention: PsimagLite's ContinuedFraction was not at hand to compare with.  z: scalar or array of complex frequencies."""
    a = np.ascontiguousarray(record["a"], np.float64)
    b = np.ascontiguousarray(record["b"], np.float64)
    if len(b) < len(a):
        b = np.concatenate([b, np.zeros(len(a) - len(b))])
    zs = np.atleast_1d(np.asarray(z, np.complex128))
    out = np.zeros(zs.shape, np.complex128)
    if len(a) == 0 and float(record["weight"]) == 0.0:  # a modified state of zero norm (spectral_function_weighted): no decomposition, G = 0
        return out if np.ndim(z) else out[0]
    o = np.zeros(2)
    lib = _capi.lib()
    for k, zz in enumerate(zs.ravel()):
        check(lib.lpp_continued_fraction(len(a), _vp(a), _vp(b), float(record["Eg"]), float(record["weight"]), float(record["sigma"]), zz.real, zz.imag, _vp(o)))
        out.ravel()[k] = complex(o[0], o[1])
    return out if np.ndim(z) else out[0]


def partition_rows(nrows, nranks, block=1):
    starts = np.zeros(nranks + 1, np.int64)
    check(_capi.lib().lpp_partition_rows(nrows, nranks, block, _vp(starts)))
    return starts


def split_csr(rank, nranks, shard_starts, shard_stride, rowptr, colind, values):
    """Split a row block (global columns) into local-column and remote-column CSRs."""
    L = _capi.lib()
    shard_starts = np.ascontiguousarray(shard_starts, np.int64)
    rowptr = np.ascontiguousarray(rowptr, np.int64)
    colind = np.ascontiguousarray(colind, np.int32)
    values = np.ascontiguousarray(values)
    local_rows = len(rowptr) - 1
    esz = values.dtype.itemsize
    nl, nr = C.c_int64(), C.c_int64()
    check(L.lpp_split_csr(rank, nranks, _vp(shard_starts), shard_stride, local_rows, _vp(rowptr), _vp(colind),
                          _vp(values), esz, C.byref(nl), C.byref(nr), None, None, None, None, None, None))
    rpl, rpr = np.zeros(local_rows + 1, np.int64), np.zeros(local_rows + 1, np.int64)
    cl, cr = np.zeros(nl.value, np.int32), np.zeros(nr.value, np.int32)
    vl, vr = np.zeros(nl.value, values.dtype), np.zeros(nr.value, values.dtype)
    check(L.lpp_split_csr(rank, nranks, _vp(shard_starts), shard_stride, local_rows, _vp(rowptr), _vp(colind),
                          _vp(values), esz, C.byref(nl), C.byref(nr), _vp(rpl), _vp(cl), _vp(vl), _vp(rpr), _vp(cr),
                          _vp(vr)))
    return (rpl, cl, vl), (rpr, cr, vr)


def tridiag_lowest(d, e, k=1, vectors=False):
    d = np.ascontiguousarray(d, np.float64)
    n = len(d)
    e2 = np.zeros(max(n, 1), np.float64)
    e2[:max(n - 1, 0)] = np.asarray(e, np.float64)[:max(n - 1, 0)]
    w = np.zeros(k)
    z = np.zeros((n, k)) if vectors else None
    check(_capi.lib().lpp_tridiag_lowest(n, _vp(d), _vp(e2), k, _vp(w), _vp(z)))
    return (w, z) if vectors else w
