// EngineGpu.h -- the reference's template concepts for the stored-CSR path, backed by the C ABI
// (include/lpp_engine.h).  Class and member names follow the reference so a maintainer can map them 1:1:
//   DefaultSymmetry        src/Engine/DefaultSymmetry.h:41-116   (owns the CSR, init() -> model.setupHamiltonian)
//   InternalProductStored  src/Engine/InternalProductStored.h:93-132 (rows(), matrixVectorProduct: x += H y)
//   ParametersForSolver    [PsimagLite] as used at src/Engine/Engine.h:609 and src/SpinOrbital.cpp:213-216
//   LanczosSolver          [PsimagLite] computeAllStatesBelow / decomposition / computeOneState
//   Engine                 src/Engine/Engine.h:84-98,601-657 (ground state), :134-206 spectralFunction, :266-338 twoPoint
//   LabeledOperator        src/Engine/LabeledOperator.h:10-119
//   ContinuedFraction(Collection)  [PsimagLite] as used at Engine.h:188,204,489 and LanczosDriver1.h:147-179 (this project's own text layout)
// The device boundary sits between Engine and the solver: the CSR is uploaded once by
// InternalProductStored, the whole Lanczos loop runs on the GPU.  Errors surface as std::runtime_error.
#ifndef LPP_HOST_ENGINE_GPU_H
#define LPP_HOST_ENGINE_GPU_H

#include <fstream>
#include <iomanip>
#include <iostream>
#include <map>
#include <memory>

#include "../../include/lpp_engine.h"
#include "Models.h"

namespace LanczosPlusPlus {

inline void lppCheck(lpp_status st)
{
	if (st != LPP_OK) throw std::runtime_error(std::string("lpp_engine: ") + lpp_last_error());
}

template <typename T> struct LppDtype {
	enum { value = LPP_F64 };
};
template <> struct LppDtype<std::complex<double>> {
	enum { value = LPP_C128 };
};

// RAII handle of one engine (one GPU)
class EngineHandle {
public:
	explicit EngineHandle(const lpp_config& cfg) : e_(nullptr) { lppCheck(lpp_engine_create(&e_, &cfg)); }
	~EngineHandle() { lpp_engine_destroy(e_); }
	lpp_engine* get() const { return e_; }

private:
	EngineHandle(const EngineHandle&);
	EngineHandle& operator=(const EngineHandle&);
	lpp_engine* e_;
};

template <typename RealType> struct ParametersForSolver {
	// labels Lanczos{Steps,Eps,MinSteps,Options}= with the given prefix; defaults as recalled from PsimagLite
	ParametersForSolver() : steps(200), minSteps(4), tolerance(1e-12), lotaMemory(true), options("none") { }
	ParametersForSolver(LppHost::InputReadable& io, const LppHost::String& prefix) : steps(200), minSteps(4), tolerance(1e-12), lotaMemory(true), options("none")
	{
		if (io.has(prefix + "Steps=")) io.readline(steps, prefix + "Steps=");
		if (io.has(prefix + "Eps=")) io.readline(tolerance, prefix + "Eps=");
		if (io.has(prefix + "MinSteps=")) io.readline(minSteps, prefix + "MinSteps=");
		if (io.has(prefix + "Options=")) io.readline(options, prefix + "Options=");
		int x = 0;
		if (io.has(prefix + "NoSaveLanczosVectors=")) {
			io.readline(x, prefix + "NoSaveLanczosVectors=");
			lotaMemory = (x == 0);
		}
	}
	SizeType steps, minSteps;
	RealType tolerance;
	bool lotaMemory;
	LppHost::String options;
};

// rows above which the reference refuses a dense diagonalisation (DefaultSymmetry.h:82)
enum { LPP_FULLDIAG_MAX_ROWS = 4900 };

template <typename BasisType_, typename GeometryType_> class DefaultSymmetry {
public:
	typedef GeometryType_ GeometryType;
	typedef typename GeometryType::ComplexOrRealType ComplexOrRealType;
	typedef typename LppHost::Real<ComplexOrRealType>::Type RealType;
	typedef LppHost::CrsMatrix<ComplexOrRealType> SparseMatrixType;
	typedef LppHost::Matrix<ComplexOrRealType> MatrixType;
	typedef std::vector<RealType> VectorRealType;
	typedef std::vector<ComplexOrRealType> VectorType;
	typedef std::vector<VectorType> VectorVectorType;
	typedef BasisType_ BasisType;

	DefaultSymmetry(const BasisType&, const GeometryType&, LppHost::String) { }
	template <typename SomeModelType> void init(const SomeModelType& model, const BasisType& basis) { model.setupHamiltonian(matrixStored_, basis); }
	// DefaultSymmetry.h:80-93: dense LAPACK diagonalisation of the stored matrix, refused above 4900 rows
	void fullDiag(VectorRealType& eigs, MatrixType& fm) const
	{
		if (rows_ > LPP_FULLDIAG_MAX_ROWS) throw LppHost::RuntimeError("fullDiag too big\n");
		if (matrixStored_.nonZeros() == 0 && rows_ > 0) throw LppHost::RuntimeError("fullDiag: the host matrix was released\n");
		fm = LppHost::toDense(matrixStored_);
		LppHost::diag(fm, eigs, 'V');
	}
	void transform(VectorVectorType&, SizeType) { }
	SizeType sectors() const { return 1; }
	void setPointer(SizeType) { }
	LppHost::String name() const { return "default"; }
	SizeType rows() const { return matrixStored_.rows(); }
	// the matrix of the sector selected by setPointer: what InternalProductStored makes resident on the GPU
	const SparseMatrixType& storedMatrix() const { return matrixStored_; }
	// after the upload the device copy is the resident one; small matrices stay on the host for the fullDiag fallback (Engine.h:633)
	void releaseHostMatrix()
	{
		rows_ = matrixStored_.rows();
		if (rows_ > LPP_FULLDIAG_MAX_ROWS) matrixStored_.resize(matrixStored_.rows(), matrixStored_.cols());
	}

private:
	SparseMatrixType matrixStored_;
	SizeType rows_ = 0;
};

// x += H y with H resident on the GPU
template <typename ModelType_, typename SpecialSymmetryType_> class InternalProductStored {
public:
	typedef ModelType_ ModelType;
	typedef SpecialSymmetryType_ SpecialSymmetryType;
	typedef typename ModelType::BasisBaseType BasisType;
	typedef typename SpecialSymmetryType::SparseMatrixType SparseMatrixType;
	typedef typename ModelType::RealType RealType;
	typedef typename ModelType::GeometryType GeometryType;
	typedef typename GeometryType::ComplexOrRealType ComplexOrRealType;
	typedef LppHost::Matrix<ComplexOrRealType> MatrixType;
	typedef std::vector<RealType> VectorRealType;
	typedef std::vector<ComplexOrRealType> VectorType;

	static lpp_config defaultConfig()
	{
		lpp_config cfg;
		lpp_config_default(&cfg);
		cfg.dtype = LppDtype<ComplexOrRealType>::value;
		return cfg;
	}
	// the reference's two constructors (InternalProductStored.h:104-117) with the default solver configuration
	InternalProductStored(const ModelType& model, SpecialSymmetryType& rs) : rs_(rs), engine_(defaultConfig()), basis_(model.basis()), model_(&model), rows_(0), sector_(0)
	{
		rs_.init(model, model.basis());
		upload();
	}
	InternalProductStored(const ModelType& model, const BasisType& basis, SpecialSymmetryType& rs) : rs_(rs), engine_(defaultConfig()), basis_(basis), model_(&basis == &model.basis() ? &model : nullptr), rows_(0), sector_(0)
	{
		rs_.init(model, basis);
		upload();
	}
	InternalProductStored(const ModelType& model, SpecialSymmetryType& rs, const lpp_config& cfg) : rs_(rs), engine_(cfg), basis_(model.basis()), model_(&model), rows_(0), sector_(0)
	{
		rs_.init(model, model.basis());
		upload();
	}
	InternalProductStored(const ModelType& model, const BasisType& basis, SpecialSymmetryType& rs, const lpp_config& cfg) : rs_(rs), engine_(cfg), basis_(basis), model_(&basis == &model.basis() ? &model : nullptr), rows_(0), sector_(0)
	{
		rs_.init(model, basis);
		upload();
	}
	SizeType rows() const { return rows_; }
	void matrixVectorProduct(VectorType& x, const VectorType& y) const
	{
		if (x.size() != rows_ || y.size() != rows_) throw std::runtime_error("InternalProductStored::matrixVectorProduct: size mismatch\n");
		lppCheck(lpp_engine_spmv_acc(engine_.get(), x.data(), y.data()));
	}
	// InternalProductStored.h:124: the matrix of symmetry sector p becomes THE matrix (ReflectionSymmetry.h:138-190 and
	// TranslationSymmetry.h:245-268 hold one CSR per sector); here it is made resident on the GPU in place of the previous one
	void specialSymmetrySector(SizeType p)
	{
		rs_.setPointer(p);
		if (p == sector_) return;
		sector_ = p;
		upload();
	}
	// InternalProductStored.h:126-130
	void fullDiag(VectorRealType& eigs, MatrixType& fm) const { rs_.fullDiag(eigs, fm); }
	lpp_engine* engine() const { return engine_.get(); }

private:
	void upload()
	{
		const SparseMatrixType& m = rs_.storedMatrix();
		rows_ = m.rows();
		// layout hint only: the Hubbard product basis is blocked in runs of N_up states (BasisHubbardLanczos.h:59-63);
		// it holds for the whole-space matrix of a one-sector symmetry, not for symmetry-adapted sector matrices
		const BasisHubbardLanczos* hb = dynamic_cast<const BasisHubbardLanczos*>(&basis_);
		const bool whole = rs_.sectors() == 1 && hb && (SizeType)hb->size() == rows_;
		lppCheck(lpp_engine_set_row_block(engine_.get(), whole ? (int64_t)hb->sizeUp() : 0));
		describeModel(rs_.sectors() == 1 && model_ && (SizeType)model_->size() == rows_);
		lppCheck(lpp_engine_set_csr(engine_.get(), (int64_t)m.rows(), m.rowptr().data(), m.colind().data(), m.values().data()));
		rs_.releaseHostMatrix(); // the device copy is the resident one (matrices small enough for fullDiag stay)
	}
	// The matrix is handed over as the CSR the model assembled (DefaultSymmetry.h:54-57).  For the two families the engine can hold without a
	// stored matrix -- the one-orbital t-J model, the S = 1/2 Heisenberg chain -- the shim also says WHICH model it is (couplings, sector): the
	// engine regenerates the matrix from that, compares it with the CSR bit for bit and only then takes the structured form (a layout hint:
	// results never depend on it; include/lpp_engine.h, lpp_engine_set_model_*).  Whole-space matrices only.
	static double partRe(double v) { return v; }
	static double partIm(double) { return 0.0; }
	static double partRe(const std::complex<double>& v) { return v.real(); }
	static double partIm(const std::complex<double>& v) { return v.imag(); }
	void describeModel(bool whole)
	{
		lppCheck(lpp_engine_set_model_tj(engine_.get(), 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0)); // forget an earlier one
		if (!whole) return;
		const int n = (int)model_->geometry().numberOfSites();
		const typename BasisType::PairIntType parts = basis_.parts();
		if (const TjMultiOrb<ComplexOrRealType>* tj = dynamic_cast<const TjMultiOrb<ComplexOrRealType>*>(model_)) {
			std::vector<double> hr((size_t)n * n), hi((size_t)n * n);
			bool cplx = false;
			for (size_t k = 0; k < hr.size(); k++) {
				hr[k] = partRe(tj->hoppings()[k]);
				hi[k] = partIm(tj->hoppings()[k]);
				cplx |= hi[k] != 0;
			}
			const std::vector<RealType>& pv = tj->potentialV;
			lppCheck(lpp_engine_set_model_tj(engine_.get(), n, (int32_t)parts.first, (int32_t)parts.second, hr.data(), cplx ? hi.data() : nullptr, tj->jpm().data(),
			                                 tj->jzz().data(), tj->w().data(), pv.size() >= (size_t)2 * n ? pv.data() : nullptr, pv.size() >= (size_t)2 * n ? (int32_t)pv.size() : 0));
		} else if (const Heisenberg<ComplexOrRealType>* hs = dynamic_cast<const Heisenberg<ComplexOrRealType>*>(model_)) {
			if (hs->twiceTheSpin() != 1 || !hs->anisotropy.empty() || sizeof(ComplexOrRealType) != sizeof(double)) return;
			lppCheck(lpp_engine_set_model_heisenberg(engine_.get(), n, (int32_t)parts.second, hs->jpm().data(), hs->jzz().data(),
			                                         hs->magneticField.empty() ? nullptr : hs->magneticField.data(), (int32_t)hs->magneticField.size()));
		}
	}
	SpecialSymmetryType& rs_;
	EngineHandle engine_;
	const BasisType& basis_;
	const ModelType* model_; // null when the basis is not the model's own (observables on N +- 1 sectors)
	SizeType rows_, sector_;
};

// x += H y without a stored matrix: SolverOptions=InternalProductOnTheFly (src/Engine/InternalProductOnTheFly.h:93-133).
// In scope for the HubbardOneOrbital family (the reference's threaded HubbardHelper::matrixVectorProduct, HubbardHelper.h:105-134).
template <typename ModelType_, typename SpecialSymmetryType_> class InternalProductOnTheFly {
public:
	typedef ModelType_ ModelType;
	typedef SpecialSymmetryType_ SpecialSymmetryType;
	typedef typename ModelType::BasisBaseType BasisType;
	typedef typename ModelType::RealType RealType;
	typedef typename ModelType::GeometryType GeometryType;
	typedef typename GeometryType::ComplexOrRealType ComplexOrRealType;
	typedef LppHost::Matrix<ComplexOrRealType> MatrixType;
	typedef std::vector<RealType> VectorRealType;
	typedef std::vector<ComplexOrRealType> VectorType;

	InternalProductOnTheFly(const ModelType& model, SpecialSymmetryType& rs, const lpp_config& cfg) : rs_(rs), engine_(cfg), rows_(model.size())
	{
		const HubbardOneOrbital<ComplexOrRealType>* hub = dynamic_cast<const HubbardOneOrbital<ComplexOrRealType>*>(&model);
		if (!hub) throw std::runtime_error("InternalProductOnTheFly: only Model=HubbardOneBand / HubbardOneBandExtended have an on-the-fly product\n");
		const SizeType n = model.geometry().numberOfSites();
		std::vector<double> hr(n * n), hi(n * n);
		for (SizeType k = 0; k < n * n; k++) {
			hr[k] = LppHost::real(hub->hoppings()[k]);
			hi[k] = LppHost::imag(hub->hoppings()[k]);
		}
		const typename BasisType::PairIntType parts = model.basis().parts();
		// Model=SuperHubbardExtended: the reference's on-the-fly lambda applies setJTermOffDiagonal too (HubbardHelper.h:119-129); the engine
		// then re-derives every row from the term list per product (lpp_engine_setup_hubbard_onthefly_super)
		lppCheck(lpp_engine_setup_hubbard_onthefly_super(engine_.get(), nullptr, (int32_t)n, parts.first, parts.second, hr.data(),
		                                                 sizeof(ComplexOrRealType) == 16 ? hi.data() : nullptr, hub->hubbardU.data(), hub->potentialEffective.data(),
		                                                 hub->coulombCoupling(), hub->jCoupling()));
	}
	SizeType rows() const { return rows_; }
	void matrixVectorProduct(VectorType& x, const VectorType& y) const
	{
		if (x.size() != rows_ || y.size() != rows_) throw std::runtime_error("InternalProductOnTheFly::matrixVectorProduct: size mismatch\n");
		lppCheck(lpp_engine_spmv_acc(engine_.get(), x.data(), y.data()));
	}
	void specialSymmetrySector(SizeType p) { rs_.setPointer(p); }
	// InternalProductOnTheFly.h:125-130: no stored matrix, hence no dense fallback
	template <typename VectorRealType, typename MatrixType> void fullDiag(VectorRealType&, MatrixType&) const
	{
		throw std::runtime_error("no fullDiag possible when on the fly\n");
	}
	lpp_engine* engine() const { return engine_.get(); }

private:
	SpecialSymmetryType& rs_;
	EngineHandle engine_;
	SizeType rows_;
};

struct TridiagonalMatrix {
	std::vector<double> a_, b_;
	void resize(SizeType n)
	{
		a_.assign(n, 0.0);
		b_.assign(n, 0.0);
	}
	SizeType size() const { return a_.size(); }
	double& a(SizeType i) { return a_[i]; }
	double& b(SizeType i) { return b_[i]; }
	const double& a(SizeType i) const { return a_[i]; }
	const double& b(SizeType i) const { return b_[i]; }
};

template <typename SolverParametersType, typename MatrixType, typename VectorType> class LanczosSolver {
public:
	typedef typename VectorType::value_type ComplexOrRealType;
	typedef typename LppHost::Real<ComplexOrRealType>::Type RealType;
	typedef std::vector<RealType> VectorRealType;
	typedef std::vector<VectorType> VectorVectorType;
	typedef TridiagonalMatrix TridiagonalMatrixType;

	// The reference hands (matrix, params) to the solver AFTER the matrix object exists (Engine.h:608-610): the parameters
	// are pushed into the engine here, so both reference-style InternalProduct constructors honour LanczosSteps= etc.
	LanczosSolver(const MatrixType& mat, const SolverParametersType& params) : mat_(mat), params_(params)
	{
		const bool reortho = params_.options.find("reortho") != LppHost::String::npos;
		lppCheck(lpp_engine_set_solver(mat_.engine(), (int32_t)params_.steps, (int32_t)params_.minSteps, params_.tolerance, reortho ? 1 : 0,
		                               params_.lotaMemory ? -1 : 0));
	}

	void computeAllStatesBelow(VectorRealType& eigs, VectorVectorType& zs, const VectorType& initial, SizeType nStates)
	{
		const SizeType n = mat_.rows();
		if (initial.size() != n) throw std::runtime_error("LanczosSolver: initial vector has wrong size\n");
		eigs.resize(nStates);
		std::vector<ComplexOrRealType> flat(n * nStates);
		lpp_stats st;
		lppCheck(lpp_engine_lanczos(mat_.engine(), initial.data(), (int32_t)nStates, eigs.data(), flat.data(), &st));
		zs.assign(nStates, VectorType(n));
		for (SizeType k = 0; k < nStates; k++) std::copy(flat.begin() + k * n, flat.begin() + (k + 1) * n, zs[k].begin());
		steps_ = st.steps;
	}
	void computeOneState(RealType& energy, VectorType& z, const VectorType& initial, SizeType excited)
	{
		VectorRealType eigs;
		VectorVectorType zs;
		computeAllStatesBelow(eigs, zs, initial, excited + 1);
		energy = eigs[excited];
		z = zs[excited];
	}
	void decomposition(const VectorType& initVector, TridiagonalMatrixType& ab)
	{
		ab.resize(params_.steps + 2); // the engine holds max_steps = params_.steps (set in the constructor) and writes at most that many
		int32_t n = 0;
		lppCheck(lpp_engine_decomposition(mat_.engine(), initVector.data(), &n, &ab.a(0), &ab.b(0), nullptr));
		ab.a_.resize(n);
		ab.b_.resize(n);
		steps_ = n;
	}
	SizeType steps() const { return steps_; }

private:
	const MatrixType& mat_;
	const SolverParametersType& params_;
	SizeType steps_ = 0;
};

// LabeledOperator (LabeledOperator.h:10-119): the operator names of -g / -c, numbered as LPP_OP_*
class LabeledOperator {
public:
	explicit LabeledOperator(const LppHost::String& s) : id_(toId(s)) { }
	explicit LabeledOperator(int id) : id_(id) { }
	int id() const { return id_; }
	LppHost::String toString() const
	{
		static const char* names[] = { "", "c", "sz", "cdagger", "n", "splus", "sminus" };
		return names[id_];
	}
	bool needsNewBasis() const { return id_ != LPP_OP_N && id_ != LPP_OP_SZ; } // :83-90
	bool isFermionic() const { return id_ == LPP_OP_C || id_ == LPP_OP_CDAGGER; } // :100-105
	SizeType numberOfTypes() const { return 4; }
	LabeledOperator transposeConjugate() const // :107-119
	{
		switch (id_) {
		case LPP_OP_C: return LabeledOperator(LPP_OP_CDAGGER);
		case LPP_OP_CDAGGER: return LabeledOperator(LPP_OP_C);
		case LPP_OP_SPLUS: return LabeledOperator(LPP_OP_SMINUS);
		case LPP_OP_SMINUS: return LabeledOperator(LPP_OP_SPLUS);
		default: return *this;
		}
	}

private:
	static int toId(const LppHost::String& s) // :36-59
	{
		if (s == "c") return LPP_OP_C;
		if (s == "sz") return LPP_OP_SZ;
		if (s == "cdagger") return LPP_OP_CDAGGER;
		if (s == "n") return LPP_OP_N;
		if (s == "splus") return LPP_OP_SPLUS;
		if (s == "sminus") return LPP_OP_SMINUS;
		throw std::runtime_error("LabeledOperator: unsupported operator " + s + " (c, cdagger, n, sz, splus, sminus)\n");
	}
	int id_;
};

// One record of a spectral function: the argument list of cf.set (Engine.h:489) and, through lpp_continued_fraction, its value at complex z.
// The text layout written here is this project's own; PsimagLite's writer was not available to compare with.
class ContinuedFraction {
public:
	typedef TridiagonalMatrix TridiagonalMatrixType;
	void set(const TridiagonalMatrix& ab, double Eg, double weight, int isign)
	{
		ab_ = ab;
		Eg_ = Eg;
		weight_ = weight;
		isign_ = isign;
	}
	std::complex<double> operator()(const std::complex<double>& z) const
	{
		double out[2] = { 0, 0 };
		lppCheck(lpp_continued_fraction((int32_t)ab_.size(), ab_.a_.data(), ab_.b_.data(), Eg_, weight_, (double)isign_, z.real(), z.imag(), out));
		return std::complex<double>(out[0], out[1]);
	}
	void write(std::ostream& os) const
	{
		os << std::setprecision(17);
		os << "#Avector " << ab_.size();
		for (SizeType k = 0; k < ab_.size(); k++) os << " " << ab_.a(k);
		os << "\n#Bvector " << ab_.size();
		for (SizeType k = 0; k < ab_.size(); k++) os << " " << ab_.b(k);
		os << "\n#CFEnergy=" << Eg_ << "\n#CFWeight=" << weight_ << "\n#CFIsign=" << isign_ << "\n";
	}
	const TridiagonalMatrix& ab() const { return ab_; }
	double energy() const { return Eg_; }
	double weight() const { return weight_; }
	int isign() const { return isign_; }

private:
	TridiagonalMatrix ab_;
	double Eg_ = 0, weight_ = 0;
	int isign_ = 1;
};

template <typename ContinuedFractionType_> class ContinuedFractionCollection {
public:
	typedef ContinuedFractionType_ ContinuedFractionType;
	void push(const ContinuedFractionType& cf) { data_.push_back(cf); }
	SizeType size() const { return data_.size(); }
	const ContinuedFractionType& operator[](SizeType k) const { return data_[k]; }
	void write(std::ostream& os) const
	{
		os << "#ContinuedFractionCollection=" << data_.size() << "\n";
		for (SizeType k = 0; k < data_.size(); k++) {
			os << "#ContinuedFraction=" << k << "\n";
			data_[k].write(os);
		}
	}

private:
	std::vector<ContinuedFractionType> data_;
};

// deterministic stand-in for PsimagLite::fillRandom (Engine.h:621): splitmix64 -> uniform(-0.5, 0.5), seed 1234
template <typename VectorType> void fillRandom(VectorType& v, uint64_t seed = 1234)
{
	typedef typename VectorType::value_type T;
	const SizeType ncomp = sizeof(T) / sizeof(double);
	double* p = reinterpret_cast<double*>(v.data());
	for (SizeType k = 0; k < v.size() * ncomp; k++) {
		uint64_t z = seed * 0x2545F4914F6CDD1DULL + k + 0x9E3779B97F4A7C15ULL;
		z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
		z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
		z ^= z >> 31;
		p[k] = (double)(z >> 11) * (1.0 / 9007199254740992.0) - 0.5;
	}
}

template <typename ModelType_, template <typename, typename> class InternalProductTemplate, typename SpecialSymmetryType_> class Engine {
public:
	typedef ModelType_ ModelType;
	typedef SpecialSymmetryType_ SpecialSymmetryType;
	typedef InternalProductTemplate<ModelType, SpecialSymmetryType> InternalProductType;
	typedef typename ModelType::RealType RealType;
	typedef typename ModelType::ComplexOrRealType ComplexOrRealType;
	typedef std::vector<ComplexOrRealType> VectorType;
	typedef std::vector<VectorType> VectorVectorType;
	typedef std::vector<RealType> VectorRealType;
	typedef ParametersForSolver<RealType> ParametersForSolverType;
	typedef LanczosSolver<ParametersForSolverType, InternalProductType, VectorType> LanczosSolverType;
	typedef typename LanczosSolverType::TridiagonalMatrixType TridiagonalMatrixType;

	Engine(const ModelType& model, LppHost::InputReadable& io, int device = 0) : model_(model), io_(io), device_(device), fam_(resolveFamily())
	{
		SizeType excited = 0;
		if (io_.has("Excited=")) io_.readline(excited, "Excited=");
		computeAllStatesBelow(excited); // Engine.h:91-97
	}
	RealType energies(SizeType ind) const { return energies_[ind]; }
	const VectorType& eigenvector(SizeType ind) const { return vectors_[ind]; }
	SizeType lanczosSteps() const { return steps_; }
	SizeType sector() const { return sector_; } // the symmetry sector the returned states live in
	bool usedFullDiag() const { return usedFullDiag_; }
	typedef std::pair<SizeType, SizeType> PairType;
	typedef std::vector<LppHost::String> VectorStringType;
	typedef LabeledOperator LabeledOperatorType;
	// N +- 1 sector Hamiltonians assembled so far by spectralFunction: they are kept, keyed by (nup, ndown) (the reference re-assembles per call, :186-187)
	SizeType sectorAssemblies() const { return sectorAssemblies_; }

	// Engine::twoPoint for a list of spin pairs (Engine.h:251-261)
	void twoPoint(LppHost::Matrix<ComplexOrRealType>& result, const LabeledOperatorType& lOperator, const std::vector<PairType>& spins, const PairType& orbs,
	              const PairType& braAndKet) const
	{
		for (SizeType i = 0; i < spins.size(); i++) {
			std::cout << "spins=" << spins[i].first << " " << spins[i].second << "\n";
			twoPoint(result, lOperator, spins[i], orbs, braAndKet);
		}
	}

	// Engine::twoPoint (Engine.h:266-338) on the resident states of the GPU engine: result(i, j) = (A_j^{spins.second} bra) . (A_i^{spins.first} ket),
	// -100 where the operator leads to no sector, the trace printed as MatrixDiagonal (:337)
	void twoPoint(LppHost::Matrix<ComplexOrRealType>& result, const LabeledOperatorType& lOperator, const PairType& spins, const PairType& orbs,
	              const PairType& braAndKet) const
	{
		lpp_engine* e = observableEngine("twoPoint");
		if (orbs.first != 0 || orbs.second != 0) throw std::runtime_error("twoPoint: one orbital only\n");
		checkBraOrKet("bra", braAndKet.first);
		checkBraOrKet("ket", braAndKet.second);
		const SizeType total = model_.geometry().numberOfSites();
		if (result.n_row() != total || result.n_col() != total) result.resize(total, total);
		std::vector<ComplexOrRealType> flat(total * total);
		ComplexOrRealType sum = 0;
		std::cout << "orbs=" << orbs.first << " " << orbs.second << "\n";
		lppCheck(fam_.two_point(e, lOperator.id(), (int32_t)spins.first, (int32_t)spins.second, (int32_t)total, (int32_t)fam_.parts.first, (int32_t)fam_.parts.second,
		                        (int32_t)braAndKet.first, (int32_t)braAndKet.second, flat.data(), &sum));
		for (SizeType i = 0; i < total; i++)
			for (SizeType j = 0; j < total; j++) result(i, j) = flat[i * total + j];
		std::cout << "MatrixDiagonal = " << sum << "\n";
	}

	typedef std::vector<SizeType> VectorSizeType;

	// Engine::manyPoint (Engine.h:341-389) on the resident states: conj(bra) . (what[n-1] ... what[0] ket), what[0] acting first, each step
	// accModifiedState_ through the sectors of hasNewParts; 0 where a step leads to no sector or the string ends in another sector.  The whole string
	// is ONE pass of the bracket kernel (lpp_engine_many_point), no intermediate vector.  n and sz act in the sector the string has reached (the
	// reference's getNeededBasis hands them the original sector's basis, ill-defined once the string has left it).  Orbital 0 only.
	// Model=Heisenberg with HeisenbergTwiceS=1: the same through the S = 1/2 family's many-point call -- n, sz, splus, sminus as BasisHeisenberg::getBraIndex has them
	// (sz is the raw 1 - 2 bit); where the reference throws (c / cdagger, S+ met in the all-up sector, S- in the all-down one) LPP_ERR_INVALID is thrown.
	// Model=TjMultiOrb with Orbitals=1 and the SolverOptions token TjOperatorStrings: the same through the t-J family's many-point call -- the operators as
	// BasisTjMultiOrbLanczos::getBraIndex has them (sz is n of the given spin); without the token the model is refused by its name.
	ComplexOrRealType manyPoint(const VectorSizeType& sites, const std::vector<LabeledOperatorType>& what, const VectorSizeType& spins, const VectorSizeType& orbs,
	                            const PairType& braAndKet) const
	{
		lpp_engine* e = stringEngine("manyPoint", true);
		if (what.size() != sites.size() || spins.size() != sites.size() || orbs.size() != sites.size()) throw std::runtime_error("manyPoint: sites, operators, spins and orbitals differ in number\n");
		checkBraOrKet("ket", braAndKet.second);
		checkBraOrKet("bra", braAndKet.first);
		std::vector<int32_t> ops(sites.size()), st(sites.size()), sp(sites.size());
		for (SizeType i = 0; i < sites.size(); i++) {
			if (orbs[i] != 0) throw std::runtime_error("manyPoint: one orbital only\n");
			ops[i] = what[i].id();
			st[i] = (int32_t)sites[i];
			sp[i] = (int32_t)spins[i];
		}
		return bracket(e, LPP_STRING_MANY_POINT, ops, st, sp, std::vector<int32_t>(sites.size(), 0), braAndKet);
	}

	// Engine::measure (Engine.h:208-249): braOpKet = { "<bra", "op;op;...", "ket>" } as the driver splits "<gs|op;op|gs>" at '|'; the product goes through
	// ModelBase::rahulMethod's rules (the LAST operator acts first) in one pass of the bracket kernel, and "bra|meas|ket = value" is printed (:248).
	// Token grammar (PsimagLite's OneOperatorSpec was not at hand; restated from its use in :221-232, UNVERIFIED): label, an optional ?dof, an optional '
	// for transpose (after the label or after the dof), the site in square brackets -- n?0[0], c'[2], c?1'[3].  bra and ket: gs.
	void measure(const VectorStringType& braOpKet) const
	{
		if (braOpKet.size() != 3) throw std::runtime_error("LanczosDriver1: Only dressed brakets allowed (FATAL ERROR)\n");
		lpp_engine* e = stringEngine("measure");
		const LppHost::String meas = braOpKet[1];
		std::vector<int32_t> ops, st, sp, fl;
		std::istringstream all(meas);
		LppHost::String tok;
		while (std::getline(all, tok, ';')) {
			const SizeType open = tok.find('['), close = tok.find(']');
			if (open == LppHost::String::npos || close == LppHost::String::npos || close < open + 2 || close + 1 != tok.size())
				throw std::runtime_error("Operator " + tok + " needs a site in brackets\n");
			const LppHost::String siteString = tok.substr(open + 1, close - open - 1);
			if (siteString.find_first_not_of("0123456789") != LppHost::String::npos) throw std::runtime_error("Operator " + tok + ": the site must be a number\n");
			LppHost::String root = tok.substr(0, open);
			bool transpose = false;
			if (!root.empty() && root.back() == '\'') {
				transpose = true;
				root.pop_back();
			}
			int dof = 0;
			const SizeType q = root.find('?');
			if (q != LppHost::String::npos) {
				const LppHost::String d = root.substr(q + 1);
				if (d != "0" && d != "1") throw std::runtime_error("Operator " + tok + ": the dof is 0 (up) or 1 (down)\n");
				dof = d == "1";
				root = root.substr(0, q);
			}
			if (!root.empty() && root.back() == '\'') {
				transpose = true;
				root.pop_back();
			}
			int label = -1; // RahulOperator::fromString (RahulOperator.h:56-63)
			if (root == "c") label = LPP_OP_C;
			else if (root == "identity") label = LPP_OP_IDENTITY;
			else if (root == "sz") label = LPP_OP_SZ;
			else if (root == "n") label = LPP_OP_N;
			else throw std::runtime_error("RahulOperator: Unknow label " + root + "\n");
			ops.push_back(label);
			st.push_back(atoi(siteString.c_str()));
			sp.push_back(dof);
			fl.push_back(transpose ? 1 : 0);
		}
		const SizeType ketIndex = levelIndex(braOpKet[2], '>'), braIndex = levelIndex(braOpKet[0], '<');
		checkBraOrKet("ket", ketIndex);
		checkBraOrKet("bra", braIndex);
		const ComplexOrRealType result = bracket(e, LPP_STRING_MEASURE, ops, st, sp, fl, PairType(braIndex, ketIndex));
		std::cout << braOpKet[0] << "|" << meas << "|" << braOpKet[2] << " = " << result << "\n";
	}

	// Engine::spectralFunction for a list of spin pairs, as the driver calls it (LanczosDriver1.h:165-171)
	template <typename ContinuedFractionCollectionType>
	void spectralFunction(ContinuedFractionCollectionType& cfCollection, VectorStringType& vstr, const LabeledOperatorType& lOperator1, int isite, int jsite,
	                      const std::vector<PairType>& spins, const PairType& orbs) const
	{
		for (SizeType i = 0; i < spins.size(); i++) spectralFunction(cfCollection, vstr, lOperator1, isite, jsite, spins[i], orbs);
	}

	// Engine::spectralFunction (Engine.h:134-206): per type the modified state is built on the device from the resident ground state, the engine of
	// the operator's sector (device-assembled once from the model's parameters) decomposes it with the Spectral solver parameters (calcSpectral :460-490)
	template <typename ContinuedFractionCollectionType>
	void spectralFunction(ContinuedFractionCollectionType& cfCollection, VectorStringType& vstr, const LabeledOperatorType& lOperator1, int isite, int jsite,
	                      const PairType& spins, const PairType& orbs) const
	{
		if (spins.first != spins.second) throw std::runtime_error("spectralFunction: no support yet for off-diagonal spin\n");
		if (orbs.first != 0 || orbs.second != 0) throw std::runtime_error("spectralFunction: one orbital only\n");
		lpp_engine* e = observableEngine("spectralFunction");
		const LabeledOperatorType lOperator2 = lOperator1.transposeConjugate();
		// refused before any sector engine is assembled; the Heisenberg model decomposes them in its own sector (needsNewBasis() is false, Engine.h:172-174)
		if (!lOperator1.needsNewBasis() && !fam_.heis) throw std::runtime_error("spectralFunction: operators that stay in the sector (n, sz) are not supported\n");
		const int n = (int)model_.geometry().numberOfSites();
		if (isite < 0 || jsite < 0 || isite >= n || jsite >= n) throw std::runtime_error("spectralFunction: site out of range\n");
		const bool isDiagonal = (isite == jsite);
		const int32_t spin = (int32_t)spins.first, nup = (int32_t)fam_.parts.first, ndown = (int32_t)fam_.parts.second;
		ParametersForSolverType params(io_, "Spectral");
		for (SizeType type = 0; type < lOperator1.numberOfTypes(); ++type) {
			if (isDiagonal && type > 1) continue;
			const LabeledOperatorType& lOperator = (type & 1) ? lOperator1 : lOperator2;
			int32_t nup2 = 0, ndown2 = 0;
			if (!newSector(lOperator, spin, n, nup2, ndown2)) continue;
			decomposeAndPush(cfCollection, vstr, "spectralFunction", lOperator, type, ((type > 1) ? -1 : 1) * (isDiagonal ? 1 : 0.5),
			                 std::to_string(spins.first) + "," + std::to_string(type) + "," + std::to_string(orbs.first) + "," + std::to_string(orbs.second), nup2, ndown2, params,
			                 [&](lpp_engine* sector, double* weight, int32_t* nsteps, double* a, double* b) {
				                 return fam_.spectral_decomposition(e, 0, sector, lOperator.id(), isite, jsite, spin, type > 1 ? -1.0 : 1.0, n, nup, ndown, weight, nsteps, a, b, nullptr);
			                 });
		}
	}

	// The momentum-resolved spectral function (this project's own definition, lpp_engine_spectral_decomposition_sum): the continued fractions of
	// |phi> = sum_r weights[r] A_r |gs>, built in one pass on the device.  Records follow spectralFunction's diagonal types: type 0 is the transpose-conjugate
	// operator with conjugated weights, type 1 the operator with the given weights; weight = s2 <phi|phi>, sigma = -s, s2 = s for a bosonic operator; the
	// state is built once (no doubling).  n and sz stay in the sector and decompose there, for every model; no elastic line is subtracted.  A real engine
	// splits complex weights: |phi> = C + i S with real C, S and <phi|G|phi> = G_CC + G_SS, one record per non-zero part, labelled "...,re" / "...,im":
	// the spectral function of a type is the sum of its records.
	template <typename ContinuedFractionCollectionType>
	void spectralFunctionWeighted(ContinuedFractionCollectionType& cfCollection, VectorStringType& vstr, const LabeledOperatorType& lOperator1,
	                              const std::vector<std::complex<double>>& weights, const std::vector<PairType>& spins) const
	{
		lpp_engine* e = observableEngine("spectralFunctionWeighted");
		const int n = (int)model_.geometry().numberOfSites();
		if ((int)weights.size() != n) throw std::runtime_error("spectralFunctionWeighted: one weight per site\n");
		const LabeledOperatorType lOperator2 = lOperator1.transposeConjugate();
		const int32_t nup = (int32_t)fam_.parts.first, ndown = (int32_t)fam_.parts.second;
		const bool isReal = std::is_same<ComplexOrRealType, double>::value;
		ParametersForSolverType params(io_, "Spectral");
		for (SizeType si = 0; si < spins.size(); si++) {
			if (spins[si].first != spins[si].second) throw std::runtime_error("spectralFunctionWeighted: no support yet for off-diagonal spin\n");
			const int32_t spin = (int32_t)spins[si].first;
			for (SizeType type = 0; type < 2; ++type) {
				const LabeledOperatorType& lOperator = (type & 1) ? lOperator1 : lOperator2;
				int32_t nup2 = 0, ndown2 = 0;
				if (!newSector(lOperator, spin, n, nup2, ndown2)) continue;
				std::vector<double> wr((size_t)n), wi((size_t)n);
				bool anyIm = false;
				for (int r = 0; r < n; r++) {
					wr[(size_t)r] = weights[(size_t)r].real();
					wi[(size_t)r] = (type & 1) ? weights[(size_t)r].imag() : -weights[(size_t)r].imag();
					anyIm = anyIm || wi[(size_t)r] != 0.0;
				}
				const bool split = isReal && anyIm;
				for (int part = 0; part < (split ? 2 : 1); part++) {
					std::vector<double> pr = (split && part == 1) ? wi : wr, pi = split ? std::vector<double>((size_t)n, 0.0) : wi;
					if (split && std::all_of(pr.begin(), pr.end(), [](double v) { return v == 0.0; })) continue;
					decomposeAndPush(cfCollection, vstr, "spectralFunctionWeighted", lOperator, type, 1,
					                 std::to_string(spin) + "," + std::to_string(type) + ",0,0" + (split ? (part ? ",im" : ",re") : ""), nup2, ndown2, params,
					                 [&](lpp_engine* sector, double* weight, int32_t* nsteps, double* a, double* b) {
						                 return fam_.spectral_decomposition_sum(e, 0, sector, lOperator.id(), spin, n, nup, ndown, n, pr.data(), pi.data(), weight, nsteps, a, b, nullptr);
					                 });
				}
			}
		}
	}

	// ReducedDensityMatrix (ReducedDensityMatrix.h:40-76) of the resident ground state for the lattice cut at `split` (sites 0 .. split-1 kept), as the
	// blocks of fixed particle numbers (k_up, k_down) in the kept sites: rho(r, c) = sum over the environment of conj(psi(alpha[r], beta)) psi(alpha[c], beta)
	// -- the conjugate on the row index (:73).  The Hubbard family, for which the states are resident; other models throw, as the reference's unpack does (:87).
	struct RdmBlockType {
		int kUp = 0, kDown = 0;
		std::vector<SizeType> alpha; // the reference's row index of every row: lo_up + lo_down * 2^split (unpackHubbard :104-123)
		LppHost::Matrix<ComplexOrRealType> rho;
	};

	void reducedDensityMatrix(std::vector<RdmBlockType>& blocks, SizeType split) const
	{
		lpp_engine* e = observableEngine("reducedDensityMatrix", true); // (the reference's ReducedDensityMatrix does not know the t-J basis)
		const int32_t n = (int32_t)model_.geometry().numberOfSites();
		const typename ModelType::BasisBaseType::PairIntType parts = model_.basis().parts();
		const int32_t nup = (int32_t)parts.first, ndown = (int32_t)parts.second, cut = (int32_t)split;
		int32_t nb = 0;
		int64_t total = 0, rows = 0;
		lppCheck(lpp_rdm_plan(LPP_BASIS_HUBBARD, n, nup, ndown, cut, &nb, &total, &rows, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
		std::vector<lpp_rdm_block> blk((size_t)nb);
		std::vector<int64_t> alpha((size_t)rows);
		lppCheck(lpp_rdm_plan(LPP_BASIS_HUBBARD, n, nup, ndown, cut, &nb, &total, &rows, nullptr, nullptr, blk.data(), alpha.data(), nullptr, nullptr));
		lppCheck(lpp_engine_state_reduced_density_matrix(e, 0, LPP_BASIS_HUBBARD, n, nup, ndown, cut, nullptr)); // every refusal, the memory check among them
		std::vector<ComplexOrRealType> flat((size_t)total);
		lppCheck(lpp_engine_state_reduced_density_matrix(e, 0, LPP_BASIS_HUBBARD, n, nup, ndown, cut, flat.data()));
		blocks.assign((size_t)nb, RdmBlockType());
		size_t row0 = 0;
		for (size_t b = 0; b < blocks.size(); b++) {
			const SizeType d = (SizeType)(blk[b].dim_up * blk[b].dim_down);
			blocks[b].kUp = blk[b].k_up;
			blocks[b].kDown = blk[b].k_down;
			blocks[b].alpha.assign(alpha.begin() + row0, alpha.begin() + row0 + d);
			blocks[b].rho.resize(d, d);
			for (SizeType i = 0; i < d; i++)
				for (SizeType j = 0; j < d; j++) blocks[b].rho(i, j) = flat[(size_t)blk[b].offset + i * d + j];
			row0 += d;
		}
	}

private:
	void checkBraOrKet(const char* what, SizeType ind) const
	{
		if (ind >= vectors_.size()) throw std::runtime_error(std::string("Engine: ") + what + " index exceeds the states computed (Excited=)\n");
	}

	// The observable family of the model: which C entry points its resident states go through, with which counts, and the model as sectorEngine reads it.
	// resolveFamily() fills it once, in the constructor: the model and the input are held by reference for the engine's lifetime and nothing in this class
	// changes either.  A further family is one more branch there.
	struct Family {
		decltype(&lpp_engine_two_point) two_point = nullptr; // null: the model has no observables here
		decltype(&lpp_obs_new_parts) new_parts = nullptr;
		decltype(&lpp_engine_spectral_decomposition) spectral_decomposition = nullptr;
		decltype(&lpp_engine_spectral_decomposition_sum) spectral_decomposition_sum = nullptr;
		decltype(&lpp_engine_many_point) many_point = nullptr; // null: the family has no operator strings
		decltype(&lpp_engine_keep_states) keep_states = lpp_engine_keep_states;
		PairType parts; // the sector as the entry points take it: (nup, ndown); Heisenberg (szPlusConst, 0); the spin-S digit basis (twiceS, szPlusConst)
		PairType ownSector; // the key of the resident states' own sector among the sector engines: parts; the spin-S digit basis (szPlusConst, 0), as its new sectors
		// the model (one of the three is set)
		const HubbardOneOrbital<ComplexOrRealType>* hubbard = nullptr;
		const TjMultiOrb<ComplexOrRealType>* tj = nullptr; // (Orbitals=1: the only one the shim builds)
		const Heisenberg<ComplexOrRealType>* heis = nullptr;
		bool spinS = false; // heis in the spin-S digit basis: sector engines come from the any-spin assembler
		bool tjStrings = false; // the input's opt-in for operator strings of the t-J basis (the reference's InputCheck is permissive, so such an input stays valid for it)
	};

	Family resolveFamily() const
	{
		Family f;
		const Heisenberg<ComplexOrRealType>* hs = dynamic_cast<const Heisenberg<ComplexOrRealType>*>(&model_);
		if (hs && solverOption("HeisenbergSpinObservables")) {
			// The input's opt-in for the observables of the spin-S digit basis: a Model=Heisenberg input of any spin the assembler admits, AnisotropyD included
			// (the project's own definition -- the reference throws for spins above 1/2 --, sz is the true S^z; the reference's InputCheck is permissive,
			// so such an input stays valid for it).  Without the token every input behaves as before.
			f.heis = hs;
			f.spinS = true;
			f.two_point = lpp_engine_two_point_heis_spin;
			f.new_parts = lpp_obs_new_parts_heis_spin;
			f.spectral_decomposition = lpp_engine_spectral_decomposition_heis_spin;
			f.spectral_decomposition_sum = lpp_engine_spectral_decomposition_sum_heis_spin;
		} else if (hs && hs->twiceTheSpin() == 1 && hs->anisotropy.empty()) {
			// S = 1/2 only: the reference throws for higher spins (BasisHeisenberg.h:130, Heisenberg.h:223).  An input with AnisotropyD is not admitted here yet:
			// its sector engines would come from the any-spin assembler, and no driver test covers that (the Python layer does both, and is tested)
			f.heis = hs;
			f.two_point = lpp_engine_two_point_heis;
			f.new_parts = lpp_obs_new_parts_heis;
			f.spectral_decomposition = lpp_engine_spectral_decomposition_heis;
			f.spectral_decomposition_sum = lpp_engine_spectral_decomposition_sum_heis;
			f.many_point = lpp_engine_many_point_heis;
		} else if ((f.tj = dynamic_cast<const TjMultiOrb<ComplexOrRealType>*>(&model_))) {
			f.tjStrings = solverOption("TjOperatorStrings");
			f.two_point = lpp_engine_two_point_tj;
			f.new_parts = lpp_obs_new_parts_tj;
			f.spectral_decomposition = lpp_engine_spectral_decomposition_tj;
			f.spectral_decomposition_sum = lpp_engine_spectral_decomposition_sum_tj;
			f.many_point = lpp_engine_many_point_tj;
			f.keep_states = lpp_engine_keep_states_tj; // (a t-J matrix may be held in the hole-major form, which only this call lets keep its states)
		} else if ((f.hubbard = dynamic_cast<const HubbardOneOrbital<ComplexOrRealType>*>(&model_))) {
			f.two_point = lpp_engine_two_point;
			f.new_parts = lpp_obs_new_parts;
			f.spectral_decomposition = lpp_engine_spectral_decomposition;
			f.spectral_decomposition_sum = lpp_engine_spectral_decomposition_sum;
			f.many_point = lpp_engine_many_point;
		}
		if (f.two_point) {
			const typename ModelType::BasisBaseType::PairIntType parts = model_.basis().parts(); // (the Heisenberg model's are (twiceS, szPlusConst))
			f.parts = (f.heis && !f.spinS) ? PairType(parts.second, 0) : PairType(parts.first, parts.second);
			f.ownSector = f.heis ? PairType(parts.second, 0) : f.parts;
		}
		return f;
	}

	bool solverOption(const char* token) const
	{
		LppHost::String options("none");
		if (io_.has("SolverOptions=")) io_.readline(options, "SolverOptions=");
		return options.find(token) != LppHost::String::npos;
	}

	// the GPU engine that holds the resident states: the Hubbard family or (unless hubbardOnly) the one-orbital t-J model or the Heisenberg model
	// on one GPU, a one-sector symmetry, states from the device solver
	lpp_engine* observableEngine(const char* who, bool hubbardOnly = false) const
	{
		if (hubbardOnly && !fam_.hubbard)
			throw std::runtime_error(std::string(who) + ": needs a Model of the HubbardOneOrbital family solved by the GPU Lanczos (no symmetry sectors, no dense fallback)\n");
		if (!fam_.two_point || !hamiltonian_ || !statesResident_)
			throw std::runtime_error(std::string(who) + ": needs a Model of the HubbardOneOrbital family, TjMultiOrb with Orbitals=1 or Heisenberg with HeisenbergTwiceS=1 and no AnisotropyD (any spin and AnisotropyD with SolverOptions=...,HeisenbergSpinObservables) solved by the GPU Lanczos (no symmetry sectors, no dense fallback)\n");
		return hamiltonian_->engine();
	}

	// manyPoint / measure: the Hubbard product basis, and for manyPoint (manyPointOk) the S = 1/2 Heisenberg basis and, where the input opts in with the
	// SolverOptions token TjOperatorStrings, the one-orbital t-J basis (there sz is n of the given spin and splus does not read its spin, so a Hubbard
	// string carried over would silently mean something else); otherwise the t-J and Heisenberg models are refused as LPP_ERR_INVALID by the model's name
	lpp_engine* stringEngine(const char* who, bool manyPointOk = false) const
	{
		lpp_engine* e = observableEngine(who);
		if (fam_.tj && !(manyPointOk && fam_.tjStrings))
			throw std::runtime_error(std::string("LPP_ERR_INVALID: ") + who + ": not for the TjMultiOrb model, operator strings are built for the Hubbard product basis"
			                         + (manyPointOk ? "; SolverOptions=...,TjOperatorStrings opts into strings of the t-J basis (sz is then n of the given spin)\n" : "\n"));
		if (fam_.spinS)
			throw std::runtime_error(std::string("LPP_ERR_INVALID: ") + who + ": operator strings are not built for the spin-S digit basis (HeisenbergSpinObservables)\n");
		if (fam_.heis && !manyPointOk)
			throw std::runtime_error(std::string("LPP_ERR_INVALID: ") + who + ": not for the Heisenberg model, operator strings are built for the Hubbard product basis\n");
		return e;
	}

	ComplexOrRealType bracket(lpp_engine* e, int convention, const std::vector<int32_t>& ops, const std::vector<int32_t>& sites, const std::vector<int32_t>& spins,
	                          const std::vector<int32_t>& flags, const PairType& braAndKet) const
	{
		const int64_t off[2] = { 0, (int64_t)ops.size() };
		double out[2] = { 0, 0 };
		lppCheck(fam_.many_point(e, convention, 1, off, ops.data(), sites.data(), spins.data(), flags.data(), (int32_t)model_.geometry().numberOfSites(),
		                         (int32_t)fam_.parts.first, (int32_t)fam_.parts.second, (int32_t)braAndKet.first, (int32_t)braAndKet.second, out));
		if constexpr (std::is_same<ComplexOrRealType, double>::value) return out[0];
		else return ComplexOrRealType(out[0], out[1]);
	}

	// PsimagLite::GetBraOrKet as Engine::measure uses it (:234-244): "gs" is level 0; nothing else is restated here
	static SizeType levelIndex(const LppHost::String& s, char bracket)
	{
		LppHost::String name = s;
		name.erase(std::remove(name.begin(), name.end(), bracket), name.end());
		if (name != "gs") throw std::runtime_error("measure: bra and ket must be gs, not " + name + "\n");
		return 0;
	}

	// the sector an operator of a spectral function decomposes in: the family's new parts or, for one that stays, the resident states' own; false: none
	bool newSector(const LabeledOperatorType& lOperator, int32_t spin, int n, int32_t& nup2, int32_t& ndown2) const
	{
		int32_t has = 1;
		nup2 = (int32_t)fam_.ownSector.first;
		ndown2 = (int32_t)fam_.ownSector.second;
		if (lOperator.needsNewBasis()) lppCheck(fam_.new_parts(lOperator.id(), spin, n, (int32_t)fam_.parts.first, (int32_t)fam_.parts.second, &has, &nup2, &ndown2));
		return has != 0;
	}

	// One record of spectralFunction / spectralFunctionWeighted: decompose(sector engine, &weight, &steps, a, b) builds the modified state and decomposes it
	// on the engine of sector (nup2, ndown2); the record is the argument list of cf.set with s = -1 for the odd types (calcSpectral, Engine.h:481-489)
	// and s2 = scale, times s for a bosonic operator.
	template <typename ContinuedFractionCollectionType, typename DecomposeType>
	void decomposeAndPush(ContinuedFractionCollectionType& cfCollection, VectorStringType& vstr, const char* who, const LabeledOperatorType& lOperator, SizeType type,
	                      RealType scale, const LppHost::String& label, int nup2, int ndown2, const ParametersForSolverType& params, DecomposeType&& decompose) const
	{
		lpp_engine* sector = sectorEngine(nup2, ndown2, params);
		TridiagonalMatrixType ab;
		ab.resize(params.steps + 2);
		double weight = 0;
		int32_t nsteps = 0;
		lppCheck(decompose(sector, &weight, &nsteps, &ab.a(0), &ab.b(0)));
		ab.a_.resize(nsteps);
		ab.b_.resize(nsteps);
		if (std::sqrt(weight) < 1e-10) std::cerr << who << ": modifVector==0, type=" << type << "\n";
		const int s = (type & 1) ? -1 : 1;
		const RealType s2 = scale * (lOperator.isFermionic() ? 1 : s);
		typename ContinuedFractionCollectionType::ContinuedFractionType cf;
		cf.set(ab, energies_[0], weight * s2, -s);
		vstr.push_back(label);
		cfCollection.push(cf);
	}

	lpp_engine* sectorEngine(int nup, int ndown, const ParametersForSolverType& params) const
	{
		std::unique_ptr<EngineHandle>& slot = sectorEngines_[PairType(nup, ndown)];
		if (!slot) {
			const HubbardOneOrbital<ComplexOrRealType>* hub = fam_.hubbard;
			const TjMultiOrb<ComplexOrRealType>* tj = fam_.tj;
			const Heisenberg<ComplexOrRealType>* hs = fam_.heis;
			const SizeType n = model_.geometry().numberOfSites();
			std::vector<double> hr(n * n), hi(n * n);
			for (SizeType k = 0; k < n * n && !hs; k++) {
				hr[k] = LppHost::real(hub ? hub->hoppings()[k] : tj->hoppings()[k]);
				hi[k] = LppHost::imag(hub ? hub->hoppings()[k] : tj->hoppings()[k]);
			}
			lpp_config cfg;
			lpp_config_default(&cfg);
			cfg.device = device_;
			cfg.dtype = LppDtype<ComplexOrRealType>::value;
			std::unique_ptr<EngineHandle> fresh(new EngineHandle(cfg));
			if (fam_.spinS) { // the recorded model's twiceS and anisotropy on szPlusConst +- 1 (or the state's own sector for sz)
				lppCheck(lpp_engine_assemble_heisenberg_spin(fresh->get(), (int32_t)n, (int32_t)hs->twiceTheSpin(), nup, hs->jpm().data(), hs->jzz().data(),
				                                             hs->magneticField.empty() ? nullptr : hs->magneticField.data(), (int32_t)hs->magneticField.size(),
				                                             hs->anisotropy.empty() ? nullptr : hs->anisotropy.data(), (int32_t)hs->anisotropy.size()));
			} else if (hs) {
				const double* field = hs->magneticField.empty() ? nullptr : hs->magneticField.data();
				lppCheck(lpp_engine_assemble_heisenberg(fresh->get(), (int32_t)n, nup, hs->jpm().data(), hs->jzz().data(), field, (int32_t)hs->magneticField.size()));
			} else if (hub) {
				lppCheck(lpp_engine_assemble_hubbard_super(fresh->get(), nullptr, (int32_t)n, nup, ndown, hr.data(), sizeof(ComplexOrRealType) == 16 ? hi.data() : nullptr,
				                                           hub->hubbardU.data(), hub->potentialEffective.data(), hub->coulombCoupling(), hub->jCoupling()));
			} else {
				const std::vector<RealType>& pv = tj->potentialV; // (as describeModel hands it over)
				const bool havePv = pv.size() >= (size_t)2 * n;
				lppCheck(lpp_engine_assemble_tj(fresh->get(), (int32_t)n, nup, ndown, hr.data(), sizeof(ComplexOrRealType) == 16 ? hi.data() : nullptr, tj->jpm().data(),
				                                tj->jzz().data(), tj->w().data(), havePv ? pv.data() : nullptr, havePv ? (int32_t)pv.size() : 0));
			}
			slot.swap(fresh);
			sectorAssemblies_++;
		}
		const bool reortho = params.options.find("reortho") != LppHost::String::npos;
		lppCheck(lpp_engine_set_solver(slot->get(), (int32_t)params.steps, (int32_t)params.minSteps, params.tolerance, reortho ? 1 : 0, 0));
		return slot->get();
	}

	// What one symmetry sector yields: its lowest levels and their vectors (sector-local), from the device solver or -- when that
	// throws -- from the dense fallback of the reference (Engine.h:627-639).
	struct SectorStates {
		VectorRealType levels;
		VectorVectorType states;
	};

	SectorStates solveSector(InternalProductType& h, LanczosSolverType& solver, SizeType nstates)
	{
		const SizeType dim = h.rows();
		SectorStates out { VectorRealType(nstates), VectorVectorType(nstates, VectorType(dim)) };
		VectorType start(dim);
		fillRandom(start); // Engine.h:621
		try {
			solver.computeAllStatesBelow(out.levels, out.states, start, nstates); // Engine.h:626
			steps_ = solver.steps();
			return out;
		} catch (std::exception& ex) {
			std::cerr << "Engine: Lanczos Solver failed (" << ex.what() << ") trying exact diagonalization...\n";
		}
		if (nstates > dim) throw std::runtime_error("Engine: more states requested than the sector holds\n");
		typename InternalProductType::VectorRealType all(dim);
		typename InternalProductType::MatrixType vecs;
		h.fullDiag(all, vecs);
		for (SizeType k = 0; k < nstates; ++k) {
			out.levels[k] = all[k];
			for (SizeType r = 0; r < dim; ++r) out.states[k][r] = vecs(r, k);
		}
		usedFullDiag_ = true;
		return out;
	}

	// Engine::computeAllStatesBelow (Engine.h:601-657): every sector of the symmetry is solved for `excited` + 1 states; the sector whose
	// lowest level is the lowest overall supplies energies_ and vectors_, which the symmetry then maps back to the full basis.
	void computeAllStatesBelow(SizeType excited)
	{
		const SizeType nstates = excited + 1;
		ParametersForSolverType params(io_, "Lanczos");
		lpp_config cfg;
		lpp_config_default(&cfg);
		cfg.device = device_;
		cfg.dtype = LppDtype<ComplexOrRealType>::value;
		// the symmetry and the matrix object outlive this call: the GPU engine keeps the states resident for twoPoint / spectralFunction
		rs_.reset(new SpecialSymmetryType(model_.basis(), model_.geometry(), ""));
		hamiltonian_.reset(new InternalProductType(model_, *rs_, cfg));
		SpecialSymmetryType& rs = *rs_;
		InternalProductType& hamiltonian = *hamiltonian_;
		LanczosSolverType lanczosSolver(hamiltonian, params); // pushes params into the engine
		const bool keep = fam_.two_point && rs.sectors() == 1;
		if (keep) lppCheck(fam_.keep_states(hamiltonian.engine(), (int32_t)nstates));
		energies_.assign(nstates, 0);
		vectors_.assign(nstates, VectorType());
		bool have = false;
		SizeType rowsBefore = 0, bestOffset = model_.size();
		for (SizeType sec = 0; sec < rs.sectors(); ++sec) {
			hamiltonian.specialSymmetrySector(sec);
			if (hamiltonian.rows() == 0) continue; // an empty sector takes no rows either (Engine.h:619)
			SectorStates found = solveSector(hamiltonian, lanczosSolver, nstates);
			const SizeType dim = found.states[0].size();
			if (!have || found.levels[0] < energies_[0]) { // Engine.h:641-649
				energies_.swap(found.levels);
				vectors_.swap(found.states);
				bestOffset = rowsBefore;
				sector_ = sec;
				have = true;
			}
			rowsBefore += dim;
		}
		rs.transform(vectors_, bestOffset); // Engine.h:654
		statesResident_ = keep && have && !usedFullDiag_;
		for (SizeType k = 0; k < nstates; k++) { // printEnergiesAndNorms, Engine.h:666-674
			RealType nrm = 0;
			for (const ComplexOrRealType& z : vectors_[k]) nrm += LppHost::real(z * LppHost::conj(z));
			std::cout << "E[" << k << "]=" << energies_[k] << " norm=" << nrm << "\n";
		}
	}
	const ModelType& model_;
	LppHost::InputReadable& io_;
	int device_;
	const Family fam_;
	VectorRealType energies_;
	VectorVectorType vectors_;
	SizeType steps_ = 0, sector_ = 0;
	bool usedFullDiag_ = false, statesResident_ = false;
	std::unique_ptr<SpecialSymmetryType> rs_;
	std::unique_ptr<InternalProductType> hamiltonian_;
	mutable std::map<PairType, std::unique_ptr<EngineHandle>> sectorEngines_;
	mutable SizeType sectorAssemblies_ = 0;
};

} // namespace LanczosPlusPlus
#endif
