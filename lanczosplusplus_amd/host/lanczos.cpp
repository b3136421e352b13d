// lanczos.cpp -- driver with the reference's command line for this path (src/lanczos.cpp:99-226,
// src/Engine/LanczosDriver1.h:47-66): reads an InputNg-style file (the reference's TestSuite inputs work
// unmodified for the in-scope models), builds the model, runs the GPU engine, prints "Energy=".
//   lanczos -f input.inp [-p precision] [-d device] [-g operator [-k momentumIndex | -w weightsFile]] [-c operator] [-s "s1,s2;..."] [-r siteForSplit] [-M "op?site?spin;...,..."] [-m "<gs|op;op|gs>,..."]
// SolverOptions=useComplex selects complex<double> (lanczos.cpp:194-226).  -c prints the two-point matrix of the ground state, -g writes the
// continued fractions of the spectral function for the site pairs the input names (TSPSites, TSPCenter=, DoAllPairs=,
// ComputeDensityOfStates=) into <input basename><counter>.comb (LanczosDriver1.h:81-199; Hubbard family, TjMultiOrb with Orbitals=1 and Heisenberg with HeisenbergTwiceS=1 -- where `-g sz` decomposes the reference's raw 1 - 2 bit = -2 S^z --, one GPU).  -r prints the reduced density
// matrix of the lattice cut at a site, its eigenvectors, eigenvalues and the entanglement entropy (LanczosDriver1.h:201-206).  -M prints static many-point
// correlations of the ground state, one "<gs|STRING|gs>=value" per comma-separated string (LanczosDriver1.h:17-45, :208-213); -m prints measure brackets,
// "bra|meas|ket = value" (LanczosDriver1.h:69-79, Engine.h:248).  Both are for the Hubbard family on one GPU; -M also serves Heisenberg with
// HeisenbergTwiceS=1 (strings of n, sz, splus, sminus; sz is the raw 1 - 2 bit = -2 S^z).
#include <getopt.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../include/lpp_comm_rccl.h"
#include "EngineGpu.h"

using namespace LanczosPlusPlus;

// LanczosOptions (src/Engine/LanczosOptions.h): what -g, -c and -s collect
struct LanczosOptions {
	typedef std::pair<SizeType, SizeType> PairSizeType;
	LanczosOptions() : spins(1, PairSizeType(0, 0)) { }
	std::vector<LabeledOperator> gf, cicj;
	std::vector<SizeType> sites;
	std::vector<PairSizeType> spins;
	int split = -1; // -r siteForSplit (LanczosOptions.h), -1: no reduced density matrix
	LppHost::String extendedStatic; // -M
	std::vector<LppHost::String> measure; // -m, one entry per occurrence
	int momentum = -1; // -k m: the -g operators summed over the sites with f_r = exp(2 pi i m r / L) / sqrt(L), instead of the site pairs
	LppHost::String weightsFile; // -w file: the same with L lines of `re im`
	bool weighted() const { return momentum >= 0 || !weightsFile.empty(); }
};

static std::vector<LppHost::String> splitString(const LppHost::String& s, char sep)
{
	std::vector<LppHost::String> out;
	std::istringstream all(s);
	LppHost::String item;
	while (std::getline(all, item, sep))
		if (!item.empty()) out.push_back(item); // (PsimagLite::split drops empty tokens)
	return out;
}

// extendedStatic (LanczosDriver1.h:17-45): "op?site?spin[?orbital];..." -> Engine::manyPoint, printed as "<gs|STRING|gs>=value"
template <typename EngineType> static void extendedStatic(const LppHost::String& manypoint, const EngineType& engine, const typename EngineType::PairType& braAndKet)
{
	typename EngineType::VectorSizeType sites, spins, orbs;
	std::vector<LabeledOperator> whats;
	for (const LppHost::String& item : splitString(manypoint, ';')) {
		const std::vector<LppHost::String> str2 = splitString(item, '?');
		if (str2.size() < 3) throw std::runtime_error("-M option malformed\n");
		whats.push_back(LabeledOperator(str2[0]));
		sites.push_back((SizeType)atoi(str2[1].c_str()));
		spins.push_back((SizeType)atoi(str2[2].c_str()));
		orbs.push_back(str2.size() == 4 ? (SizeType)atoi(str2[3].c_str()) : 0);
	}
	std::cout << "<gs|" << manypoint << "|gs>=";
	std::cout << engine.manyPoint(sites, whats, spins, orbs, braAndKet);
	std::cout << "\n";
}

// -s "s1,s2;s1,s2;..." (lanczos.cpp:17-34, :147-152)
static void fillSpins(std::vector<LanczosOptions::PairSizeType>& spins, const LppHost::String& arg)
{
	spins.clear();
	std::istringstream all(arg);
	LppHost::String item;
	while (std::getline(all, item, ';')) {
		const SizeType comma = item.find(',');
		if (comma == LppHost::String::npos) throw std::runtime_error("-s needs pairs \"s1,s2\" separated by ;\n");
		const int s1 = atoi(item.substr(0, comma).c_str()), s2 = atoi(item.substr(comma + 1).c_str());
		if (s1 < 0 || s1 > 1 || s2 < 0 || s2 > 1) throw std::runtime_error("-s: a spin is 0 (up) or 1 (down)\n");
		spins.push_back(LanczosOptions::PairSizeType(s1, s2));
	}
	if (spins.empty()) throw std::runtime_error("-s: no spin pair given\n");
}

static LppHost::String basenameOf(const LppHost::String& path)
{
	const SizeType slash = path.find_last_of('/');
	return slash == LppHost::String::npos ? path : path.substr(slash + 1);
}

// PsimagLite::Matrix's operator<< as the reference's driver uses it (LanczosDriver1.h:196): "rows cols", then one row per line
template <typename T> static void printMatrix(std::ostream& os, const LppHost::Matrix<T>& m)
{
	os << m.n_row() << " " << m.n_col() << "\n";
	for (SizeType i = 0; i < m.n_row(); i++) {
		for (SizeType j = 0; j < m.n_col(); j++) os << m(i, j) << " ";
		os << "\n";
	}
}

// -r (LanczosDriver1.h:201-206, ReducedDensityMatrix::printAll :53-61): the matrix is block diagonal in the particle numbers (k_up, k_down) of the kept
// sites and is printed block by block -- "# block k_up= k_down= dim=", "# alpha" with the reference's row index of every row, then the block as
// printMatrix prints a matrix; blocks of more than 64 rows print their two comment lines only.  The eigenvalues of all blocks follow merged
// ascending ("count" on a line, then the values), then EntanglementEntropy= -sum lambda ln lambda over lambda > 0.
template <typename EngineType> static void printReducedDensityMatrix(std::ostream& os, const EngineType& engine, SizeType split)
{
	typedef typename EngineType::ComplexOrRealType ComplexOrRealType;
	const SizeType maxPrinted = 64;
	std::vector<typename EngineType::RdmBlockType> blocks;
	engine.reducedDensityMatrix(blocks, split);
	std::vector<LppHost::Matrix<ComplexOrRealType>> vectors(blocks.size());
	std::vector<double> all;
	for (SizeType b = 0; b < blocks.size(); b++) {
		std::vector<double> eigs;
		vectors[b] = blocks[b].rho;
		LppHost::diag(vectors[b], eigs, 'V');
		all.insert(all.end(), eigs.begin(), eigs.end());
	}
	for (int what = 0; what < 2; what++) {
		os << (what == 0 ? "Reduced Density Matrix\n" : "Eigenvectors of Reduced Density Matrix\n");
		for (SizeType b = 0; b < blocks.size(); b++) {
			const SizeType d = blocks[b].rho.n_row();
			os << "# block k_up=" << blocks[b].kUp << " k_down=" << blocks[b].kDown << " dim=" << d << "\n";
			os << "# alpha";
			for (SizeType i = 0; i < d && d <= maxPrinted; i++) os << " " << blocks[b].alpha[i];
			if (d > maxPrinted) os << " (not printed: more than " << maxPrinted << " rows)";
			os << "\n";
			if (d <= maxPrinted) printMatrix(os, what == 0 ? blocks[b].rho : vectors[b]);
		}
	}
	std::sort(all.begin(), all.end());
	os << "Eigenvalues of Reduced Density Matrix\n" << all.size() << "\n";
	double entropy = 0;
	for (SizeType i = 0; i < all.size(); i++) {
		os << all[i] << " ";
		if (all[i] > 0) entropy -= all[i] * std::log(all[i]);
	}
	os << "\nEntanglementEntropy=" << entropy << "\n";
}

// mainLoop3 (LanczosDriver1.h:47-199): build the engine, print the ground-state energy, then the observables asked for
template <typename ModelType, typename SymmetryType, template <typename, typename> class InternalProductTemplate>
int mainLoop3(const ModelType& model, LppHost::InputReadable& io, int device, int precision, LanczosOptions& lanczosOptions)
{
	typedef Engine<ModelType, InternalProductTemplate, SymmetryType> EngineType;
	typedef typename ModelType::ComplexOrRealType ComplexOrRealType;
	typedef LanczosOptions::PairSizeType PairSizeType;
	std::cout.precision(precision);
	EngineType engine(model, io, device);
	std::cout << "Energy=" << engine.energies(0) << "\n";
	std::cerr << "#LanczosSteps=" << engine.lanczosSteps() << " rows=" << model.size() << "\n";
	const LppHost::String filename = basenameOf(io.filename());
	const SizeType n = model.geometry().numberOfSites();

	// -m (LanczosDriver1.h:69-79): comma-separated brackets, each split at '|' into bra, operators, ket
	for (SizeType i = 0; i < lanczosOptions.measure.size(); ++i)
		for (const LppHost::String& token : splitString(lanczosOptions.measure[i], ',')) engine.measure(splitString(token, '|'));

	// the site pairs of -g (LanczosDriver1.h:81-136)
	bool needsDos = false;
	if (io.has("ComputeDensityOfStates=")) {
		int tmp = 0;
		io.readline(tmp, "ComputeDensityOfStates=");
		needsDos = (tmp > 0);
	}
	std::vector<PairSizeType> pairOfSites;
	if (needsDos) {
		lanczosOptions.gf.push_back(LabeledOperator("c"));
		for (SizeType i = 0; i < n; ++i) pairOfSites.push_back(PairSizeType(i, i));
	}
	if (io.has("TSPSites")) {
		io.read(lanczosOptions.sites, "TSPSites");
		if (lanczosOptions.sites.size() == 0) throw std::runtime_error("TSPSites must have at least one site\n");
		if (lanczosOptions.sites.size() == 1) lanczosOptions.sites.push_back(lanczosOptions.sites[0]);
		pairOfSites.push_back(PairSizeType(lanczosOptions.sites[0], lanczosOptions.sites[1]));
	}
	bool hasCenter = false;
	SizeType centerSite = 0;
	if (io.has("TSPCenter=")) {
		io.readline(centerSite, "TSPCenter=");
		std::cout << "TSPCenter=" << centerSite << "\n";
		for (SizeType i = 0; i < n; ++i) pairOfSites.push_back(PairSizeType(centerSite, i));
		hasCenter = true;
	}
	bool doAllPairs = false;
	if (io.has("DoAllPairs=")) {
		int tmp = 0;
		io.readline(tmp, "DoAllPairs=");
		doAllPairs = (tmp > 0);
	}
	if (doAllPairs && hasCenter) throw std::runtime_error("You cannot have both TSPCenter and DoAllPairs\n");
	if (doAllPairs)
		for (SizeType i = 0; i < n; ++i)
			for (SizeType j = 0; j < n; ++j) pairOfSites.push_back(PairSizeType(i, j));

	// -g with -k / -w: one .comb file per operator holding the continued fractions of sum_r f_r A_r |gs> (Engine::spectralFunctionWeighted), in place
	// of the site pairs; the header names the momentum or the weights' file
	if (lanczosOptions.weighted()) {
		std::vector<std::complex<double>> weights(n);
		if (lanczosOptions.momentum >= 0) {
			const double pi = std::acos(-1.0);
			// the phase is m r / L of a turn: reduced in integers, and exact on the axes, so that a commensurate momentum (m = 0, L/2; quarter turns)
			// has weights that ARE real or imaginary -- a rounding residue of sin(pi r) would otherwise pass for a weight and get a record of its own
			for (SizeType r = 0; r < n; ++r) {
				const SizeType t = ((SizeType)lanczosOptions.momentum * r) % n; // t / n of a turn
				const double a = 1.0 / std::sqrt((double)n), ph = 2.0 * pi * (double)t / (double)n;
				double re = a * std::cos(ph), im = a * std::sin(ph);
				if ((4 * t) % n == 0) { // a multiple of a quarter turn
					const SizeType q = 4 * t / n;
					re = (q == 0) ? a : (q == 2) ? -a : 0.0;
					im = (q == 1) ? a : (q == 3) ? -a : 0.0;
				}
				weights[r] = std::complex<double>(re, im);
			}
		} else {
			std::ifstream fin(lanczosOptions.weightsFile.c_str());
			if (!fin) throw std::runtime_error("lanczos: cannot read " + lanczosOptions.weightsFile + "\n");
			for (SizeType r = 0; r < n; ++r) {
				double re = 0, im = 0;
				if (!(fin >> re >> im)) throw std::runtime_error("lanczos: " + lanczosOptions.weightsFile + " must hold one line `re im` per site\n");
				weights[r] = std::complex<double>(re, im);
			}
		}
		for (SizeType gfi = 0; gfi < lanczosOptions.gf.size(); ++gfi) {
			std::cout << "#gf(weighted)\n";
			typename EngineType::VectorStringType vstr;
			ContinuedFractionCollection<ContinuedFraction> cfCollection;
			engine.spectralFunctionWeighted(cfCollection, vstr, lanczosOptions.gf[gfi], weights, lanczosOptions.spins);
			const LppHost::String outName = filename + std::to_string(gfi) + ".comb";
			std::ofstream ioOut(outName.c_str());
			if (!ioOut) throw std::runtime_error("lanczos: cannot write " + outName + "\n");
			if (lanczosOptions.momentum >= 0) ioOut << "Momentum=" << lanczosOptions.momentum << "\n";
			else ioOut << "Weights=" << lanczosOptions.weightsFile << "\n";
			ioOut << "#INDEXTOCF ";
			for (SizeType i = 0; i < vstr.size(); ++i) ioOut << vstr[i] << " ";
			ioOut << "\n";
			cfCollection.write(ioOut);
			ioOut.close();
			if (!ioOut) throw std::runtime_error("lanczos: cannot write " + outName + "\n");
			std::cerr << "lanczos: Written to " << outName << "\n";
		}
	}
	// -g (LanczosDriver1.h:138-183): one .comb file per site pair, in the working directory
	for (SizeType gfi = 0; gfi < lanczosOptions.gf.size() && !lanczosOptions.weighted(); ++gfi) {
		SizeType counter = 0;
		for (SizeType sIndex = 0; sIndex < pairOfSites.size(); ++sIndex) {
			const SizeType site0 = pairOfSites[sIndex].first, site1 = pairOfSites[sIndex].second;
			std::cout << "#gf(i=" << site0 << ", j=" << site1 << ")\n";
			typename EngineType::VectorStringType vstr;
			ContinuedFractionCollection<ContinuedFraction> cfCollection;
			engine.spectralFunction(cfCollection, vstr, lanczosOptions.gf[gfi], (int)site0, (int)site1, lanczosOptions.spins, PairSizeType(0, 0));
			const LppHost::String outName = filename + std::to_string(counter) + ".comb";
			std::ofstream ioOut(outName.c_str());
			if (!ioOut) throw std::runtime_error("lanczos: cannot write " + outName + "\n");
			ioOut << "Site0=" << site0 << "\n";
			ioOut << "Site1=" << site1 << "\n";
			if (hasCenter) ioOut << "TSPCenter=" << centerSite << "\n";
			ioOut << "#INDEXTOCF ";
			for (SizeType i = 0; i < vstr.size(); ++i) ioOut << vstr[i] << " ";
			ioOut << "\n";
			cfCollection.write(ioOut);
			ioOut.close();
			if (!ioOut) throw std::runtime_error("lanczos: cannot write " + outName + "\n");
			std::cerr << "lanczos: Written to " << outName << "\n";
			++counter;
		}
	}
	if (lanczosOptions.gf.size() > 0) std::cerr << "#SectorAssemblies=" << engine.sectorAssemblies() << "\n";

	// -c (LanczosDriver1.h:185-199)
	for (SizeType cicji = 0; cicji < lanczosOptions.cicj.size(); cicji++) {
		LppHost::Matrix<ComplexOrRealType> cicjMatrix(n, n);
		engine.twoPoint(cicjMatrix, lanczosOptions.cicj[cicji], lanczosOptions.spins, PairSizeType(0, 0), PairSizeType(0, 0));
		printMatrix(std::cout, cicjMatrix);
	}

	// -r (LanczosDriver1.h:201-206)
	if (lanczosOptions.split >= 0) printReducedDensityMatrix(std::cout, engine, (SizeType)lanczosOptions.split);

	// -M (LanczosDriver1.h:208-213)
	if (lanczosOptions.extendedStatic != "")
		for (const LppHost::String& str : splitString(lanczosOptions.extendedStatic, ',')) extendedStatic(str, engine, PairSizeType(0, 0));
	return 0;
}

template <typename ComplexOrRealType> int mainLoop0(LppHost::InputReadable& io, int device, int precision, bool onthefly, LanczosOptions& lanczosOptions)
{
	typedef LppHost::Geometry<ComplexOrRealType> GeometryType;
	typedef ModelBase<ComplexOrRealType> ModelType;
	typedef DefaultSymmetry<typename ModelType::BasisBaseType, GeometryType> SymmetryType;
	GeometryType geometry(io);
	ModelSelector<ComplexOrRealType> modelSelector(io, geometry);
	const ModelType& model = modelSelector();
	model.print(std::cout);
	// stored / on-the-fly switch on the SolverOptions substring (LanczosDriver1.h:217-239)
	if (onthefly) return mainLoop3<ModelType, SymmetryType, InternalProductOnTheFly>(model, io, device, precision, lanczosOptions);
	return mainLoop3<ModelType, SymmetryType, InternalProductStored>(model, io, device, precision, lanczosOptions);
}

static int envInt(const char* name, int dflt)
{
	const char* s = getenv(name);
	return s ? atoi(s) : dflt;
}

static void rcclCheck(lpp_status st)
{
	if (st != LPP_OK) throw std::runtime_error(std::string("lpp_comm_rccl: ") + lpp_rccl_last_error() + "\n");
}

// Rank 0 creates the id and publishes it atomically (write + rename); the others poll for the file.  The file is
//   "LPPRCCL1" | 8-byte launch nonce | 128-byte id
// and a reader accepts it only with ITS OWN launch nonce (a hash of LPP_RCCL_NONCE, else of the launcher's
// TORCHELASTIC_RUN_ID / MASTER_ADDR:MASTER_PORT, which every rank of one launch shares) and only when it is not older than
// the reader itself by more than five minutes: a file left behind by a crashed run is never joined.  Rank 0 unlinks any old
// file before it writes and removes the new one once ncclCommInitRank has returned (a collective: every rank has read it).
static const char kIdMagic[8] = { 'L', 'P', 'P', 'R', 'C', 'C', 'L', '1' };

static uint64_t launchNonce()
{
	std::string key;
	if (const char* s = getenv("LPP_RCCL_NONCE")) key = s;
	else {
		for (const char* name : { "TORCHELASTIC_RUN_ID", "MASTER_ADDR", "MASTER_PORT", "SLURM_JOB_ID", "SLURM_STEP_ID" })
			if (const char* v = getenv(name)) key += std::string(name) + "=" + v + ";";
	}
	if (key.empty()) return 0; // no launch identity: shareUniqueId refuses more than one rank
	uint64_t h = 1469598103934665603ull; // FNV-1a
	for (unsigned char c : key) h = (h ^ c) * 1099511628211ull;
	return h ? h : 1;
}

static void shareUniqueId(char* id, int rank, int world)
{
	const char* path = getenv("LPP_RCCL_ID_FILE");
	if (world > 1 && !path) throw std::runtime_error("lanczos -P: set LPP_RCCL_ID_FILE to a path every rank can read\n");
	const uint64_t nonce = launchNonce();
	// without a launch identity every launch would share one nonce and a rank could join the id file a crashed run left behind
	if (world > 1 && nonce == 0)
		throw std::runtime_error("lanczos -P: no launch identity (set LPP_RCCL_NONCE to a value unique to this launch, or start the ranks through a launcher that exports MASTER_ADDR/MASTER_PORT, TORCHELASTIC_RUN_ID or SLURM_JOB_ID)\n");
	if (rank == 0) {
		rcclCheck(lpp_rccl_unique_id(id));
		if (world == 1) return;
		(void)unlink(path); // never leave a previous run's id where a reader could find it
		const std::string tmp = std::string(path) + ".tmp";
		FILE* f = fopen(tmp.c_str(), "wb");
		const bool ok = f && fwrite(kIdMagic, 1, 8, f) == 8 && fwrite(&nonce, 1, 8, f) == 8 && fwrite(id, 1, LPP_RCCL_ID_BYTES, f) == LPP_RCCL_ID_BYTES;
		if (f) fclose(f);
		if (!ok) throw std::runtime_error("lanczos -P: cannot write the RCCL id file\n");
		if (rename(tmp.c_str(), path) != 0) throw std::runtime_error("lanczos -P: cannot publish the RCCL id file\n");
		return;
	}
	const time_t started = time(nullptr);
	for (int tries = 0; tries < 6000; tries++) { // up to 10 minutes
		FILE* f = fopen(path, "rb");
		if (f) {
			char magic[8];
			uint64_t got = 0;
			struct stat sb;
			const bool fresh = fstat(fileno(f), &sb) == 0 && sb.st_mtime + 300 >= started;
			const bool ok = fread(magic, 1, 8, f) == 8 && std::memcmp(magic, kIdMagic, 8) == 0 && fread(&got, 1, 8, f) == 8 && got == nonce
			    && fread(id, 1, LPP_RCCL_ID_BYTES, f) == LPP_RCCL_ID_BYTES;
			fclose(f);
			if (ok && fresh) return;
		}
		usleep(100000);
	}
	throw std::runtime_error("lanczos -P: timed out waiting for this launch's RCCL id file (stale files are ignored)\n");
}

static long binomial(long n, long k)
{
	if (k < 0 || k > n) return 0;
	long r = 1;
	for (long i = 1; i <= k; i++) r = r * (n - k + i) / i;
	return r;
}

// one process per GPU: this rank's rows are assembled on its GPU, the Lanczos loop runs on all ranks in lock step
// (every rank takes bitwise-identical decisions), rank 0 prints the reference's "Energy=" line
static double realPart(double v) { return v; }
static double imagPart(double) { return 0.0; }
static double realPart(const std::complex<double>& v) { return v.real(); }
static double imagPart(const std::complex<double>& v) { return v.imag(); }

// Models without a device assembler for row partitions (Heisenberg, TjMultiOrb, ...): every rank lets the model assemble its CSR on the host
// (DefaultSymmetry.h:54-57), keeps rows [rank * per, (rank + 1) * per) and hands them over with lpp_engine_set_csr_partition; the Lanczos
// vector travels by all-gather (the north_star's form).
template <typename ComplexOrRealType>
static int partitionedFromHostCsr(const ModelBase<ComplexOrRealType>& model, const ParametersForSolver<double>& params, int precision, bool isComplex)
{
	const int rank = envInt("RANK", 0), world = envInt("WORLD_SIZE", 1), local = envInt("LOCAL_RANK", rank);
	typename ModelBase<ComplexOrRealType>::SparseMatrixType h;
	model.setupHamiltonian(h);
	const int64_t rows = (int64_t)h.rows(), per = (rows + world - 1) / world;
	std::vector<int64_t> starts((size_t)world + 1);
	for (int k = 0; k <= world; k++) starts[(size_t)k] = std::min<int64_t>((int64_t)k * per, rows);
	const int64_t r0 = starts[(size_t)rank], r1 = starts[(size_t)rank + 1], p0 = h.rowptr()[(size_t)r0];
	std::vector<int64_t> rp((size_t)(r1 - r0) + 1);
	for (int64_t r = r0; r <= r1; r++) rp[(size_t)(r - r0)] = h.rowptr()[(size_t)r] - p0;
	char id[LPP_RCCL_ID_BYTES];
	shareUniqueId(id, rank, world);
	lpp_config cfg;
	lpp_config_default(&cfg);
	cfg.device = local;
	cfg.dtype = isComplex ? LPP_C128 : LPP_F64;
	cfg.max_steps = (int32_t)params.steps;
	cfg.min_steps = (int32_t)params.minSteps;
	cfg.eps = params.tolerance;
	cfg.reortho = params.options.find("reortho") != LppHost::String::npos;
	cfg.save_vectors = 0;
	EngineHandle engine(cfg);
	lpp_rccl_comm* comm = nullptr;
	rcclCheck(lpp_rccl_comm_create(&comm, rank, world, id, local, lpp_engine_stream(engine.get()), per, (int32_t)params.steps, isComplex ? 1 : 0, 0));
	if (rank == 0 && world > 1) (void)unlink(getenv("LPP_RCCL_ID_FILE"));
	rcclCheck(lpp_rccl_comm_selftest(comm));
	lppCheck(lpp_engine_set_csr_partition(engine.get(), lpp_rccl_comm_get(comm), rows, starts.data(), rp.data(), h.colind().data() + p0, h.values().data() + p0));
	double e0 = 0;
	lpp_stats st;
	lppCheck(lpp_engine_lanczos(engine.get(), nullptr, 1, &e0, nullptr, &st));
	if (rank == 0) {
		std::cout.precision(precision);
		model.print(std::cout);
		std::cout << "Energy=" << e0 << "\n";
		std::cerr << "#LanczosSteps=" << st.steps << " rows=" << rows << " ranks=" << world << " exchange=" << (world > 1 ? "allgather" : "none") << " (host CSR, row partition)\n";
	}
	lppCheck(lpp_engine_sync(engine.get()));
	rcclCheck(lpp_rccl_comm_destroy(comm));
	return 0;
}

template <typename ComplexOrRealType> static int mainPartitioned(LppHost::InputReadable& io, int precision, bool onthefly)
{
	typedef LppHost::Geometry<ComplexOrRealType> GeometryType;
	const bool isComplex = sizeof(ComplexOrRealType) == 2 * sizeof(double); // SolverOptions=useComplex (lanczos.cpp:194-226): complex vectors, hoppings with phases
	const int rank = envInt("RANK", 0), world = envInt("WORLD_SIZE", 1), local = envInt("LOCAL_RANK", rank);
	GeometryType geometry(io);
	ModelSelector<ComplexOrRealType> modelSelector(io, geometry);
	const ModelBase<ComplexOrRealType>& model = modelSelector();
	const HubbardOneOrbital<ComplexOrRealType>* hub = dynamic_cast<const HubbardOneOrbital<ComplexOrRealType>*>(&model);
	if (!hub) {
		if (onthefly) throw std::runtime_error("lanczos -P: SolverOptions=InternalProductOnTheFly is the Hubbard family's path\n");
		ParametersForSolver<double> paramsGeneric(io, "Lanczos");
		return partitionedFromHostCsr<ComplexOrRealType>(model, paramsGeneric, precision, isComplex);
	}
	const int n = (int)geometry.numberOfSites();
	const typename ModelBase<ComplexOrRealType>::BasisBaseType::PairIntType parts = model.basis().parts();
	const long n_up = binomial(n, parts.first), n_dn = binomial(n, parts.second);
	const long per = (n_dn + world - 1) / world;
	std::string exchange = hub->jCoupling() ? "allgather" : "transpose"; // spin-flip terms (SuperHubbardExtended) need the gathered vector
	if (const char* s = getenv("LPP_EXCHANGE")) exchange = s;
	const long chunk = exchange == "transpose" ? (long)lpp_xchg_chunk(n_up, n_dn, world) : 0; // up range per rank rounded to 16: product-basis kernels
	ParametersForSolver<double> params(io, "Lanczos");
	char id[LPP_RCCL_ID_BYTES];
	// everything that can throw on ONE rank comes before the communicator exists: afterwards a rank that leaves alone would
	// strand its peers inside a collective
	if (onthefly && hub->jCoupling()) throw std::runtime_error("lanczos -P: the term-list product of Model=SuperHubbardExtended runs on one GPU: use the stored engine (SolverOptions=none) with -P\n");
	shareUniqueId(id, rank, world);
	lpp_config cfg;
	lpp_config_default(&cfg);
	cfg.device = local;
	cfg.dtype = isComplex ? LPP_C128 : LPP_F64;
	cfg.max_steps = (int32_t)params.steps;
	cfg.min_steps = (int32_t)params.minSteps;
	cfg.eps = params.tolerance;
	cfg.reortho = params.options.find("reortho") != LppHost::String::npos;
	cfg.save_vectors = 0; // energies only: no vector of the full length is ever gathered
	EngineHandle engine(cfg); // engine-owned stream; the communicator is told which one below
	lpp_rccl_comm* comm = nullptr;
	rcclCheck(lpp_rccl_comm_create(&comm, rank, world, id, local, lpp_engine_stream(engine.get()), per * n_up, (int32_t)params.steps, isComplex ? 1 : 0, chunk));
	if (rank == 0 && world > 1) (void)unlink(getenv("LPP_RCCL_ID_FILE")); // ncclCommInitRank is a collective: every rank has read the id
	rcclCheck(lpp_rccl_comm_selftest(comm)); // every callback once, checked on every rank, before any step depends on them
	std::vector<double> hr((size_t)n * n), hi((size_t)n * n);
	for (int k = 0; k < n * n; k++) {
		hr[(size_t)k] = realPart(hub->hoppings()[(size_t)k]);
		hi[(size_t)k] = imagPart(hub->hoppings()[(size_t)k]);
	}
	const double* him = isComplex ? hi.data() : nullptr;
	if (onthefly)
		lppCheck(lpp_engine_setup_hubbard_onthefly_ext(engine.get(), lpp_rccl_comm_get(comm), n, parts.first, parts.second, hr.data(), him,
		                                               hub->hubbardU.data(), hub->potentialEffective.data(), hub->coulombCoupling()));
	else
		lppCheck(lpp_engine_assemble_hubbard_super(engine.get(), lpp_rccl_comm_get(comm), n, parts.first, parts.second, hr.data(), him,
		                                           hub->hubbardU.data(), hub->potentialEffective.data(), hub->coulombCoupling(), hub->jCoupling()));
	double e0 = 0;
	lpp_stats st;
	lppCheck(lpp_engine_lanczos(engine.get(), nullptr, 1, &e0, nullptr, &st));
	if (rank == 0) {
		std::cout.precision(precision);
		model.print(std::cout);
		std::cout << "Energy=" << e0 << "\n";
		std::cerr << "#LanczosSteps=" << st.steps << " rows=" << model.size() << " ranks=" << world << " exchange=" << (world > 1 ? exchange : "none") << "\n";
	}
	lppCheck(lpp_engine_sync(engine.get())); // the communicator's buffers are released next: nothing of the engine may be queued on them
	rcclCheck(lpp_rccl_comm_destroy(comm));
	return 0;
}

int main(int argc, char** argv)
{
	LppHost::String file;
	int device = 0, precision = 8, opt = 0;
	bool partitioned = false;
	const char* usage = " -f filename [-p precision] [-d device] [-P] [-g operator [-k momentumIndex | -w weightsFile]] [-c operator] [-s \"s1,s2;...\"] [-r siteForSplit] [-M \"op?site?spin;...\"] [-m \"<gs|op;op|gs>\"]\n";
	LanczosOptions lanczosOptions;
	LppHost::String spinsArg;
	std::vector<LppHost::String> gfArgs, cicjArgs;
	while ((opt = getopt(argc, argv, "f:p:d:Pg:c:s:r:M:m:k:w:")) != -1) {
		switch (opt) {
		case 'f': file = optarg; break;
		case 'g': gfArgs.push_back(optarg); break;
		case 'c': cicjArgs.push_back(optarg); break;
		case 's': spinsArg = optarg; break;
		case 'r': lanczosOptions.split = atoi(optarg); break;
		case 'M': lanczosOptions.extendedStatic = optarg; break;
		case 'm': lanczosOptions.measure.push_back(optarg); break;
		case 'k': lanczosOptions.momentum = atoi(optarg); break;
		case 'w': lanczosOptions.weightsFile = optarg; break;
		case 'p': precision = atoi(optarg); break;
		case 'd': device = atoi(optarg); break;
		case 'P': partitioned = true; break;
		default: std::cerr << "USAGE: " << argv[0] << usage; return 1;
		}
	}
	if (file.empty()) {
		std::cerr << "USAGE: " << argv[0] << usage;
		return 1;
	}
	try {
		for (const LppHost::String& g : gfArgs) lanczosOptions.gf.push_back(LabeledOperator(g));
		for (const LppHost::String& c : cicjArgs) lanczosOptions.cicj.push_back(LabeledOperator(c));
		if (!spinsArg.empty()) fillSpins(lanczosOptions.spins, spinsArg);
		if (lanczosOptions.weighted() && gfArgs.empty()) throw std::runtime_error("-k / -w give the site weights of -g: not without -g\n");
		if (lanczosOptions.momentum >= 0 && !lanczosOptions.weightsFile.empty()) throw std::runtime_error("-k and -w both give the site weights: one of them\n");
		if (partitioned && (!gfArgs.empty() || !cicjArgs.empty() || lanczosOptions.split >= 0 || !lanczosOptions.extendedStatic.empty() || !lanczosOptions.measure.empty()))
			throw std::runtime_error("-g / -c / -r / -M / -m run on one GPU: not with -P\n");
		LppHost::InputReadable io(file);
		LppHost::String options("none");
		if (io.has("SolverOptions=")) io.readline(options, "SolverOptions=");
		const bool onthefly = options.find("InternalProductOnTheFly") != LppHost::String::npos;
		const bool isComplex = options.find("useComplex") != LppHost::String::npos;
		if (partitioned) return isComplex ? mainPartitioned<std::complex<double>>(io, precision, onthefly) : mainPartitioned<double>(io, precision, onthefly);
		return isComplex ? mainLoop0<std::complex<double>>(io, device, precision, onthefly, lanczosOptions) : mainLoop0<double>(io, device, precision, onthefly, lanczosOptions);
	} catch (std::exception& e) {
		std::cerr << "lanczos: " << e.what();
		return 2;
	}
}
