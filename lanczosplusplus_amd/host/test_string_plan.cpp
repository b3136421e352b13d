// test_string_plan.cpp -- the host planner of the operator strings (csrc/lpp_obs_string_plan.h) in a stand-alone program, meant to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_many_point_host.py does).  It checks, for many strings and sectors:
//   - the tables' invariants: sizes, every entry a rank of the source sector, no source used twice;
//   - that the composed plan of a many-point string IS the composition of the one-operator plans through the sectors, destination by destination,
//     sz factors included (evaluated on the words of the sector each operator meets);
//   - the upload images (StringImage): one string as apply uploads it and batches of 1, 8 and 5 in the 8 slots of the bracket kernel, every table,
//     word list and sz word read back against its plan; a table that is not of the image's species count is refused, not copied;
//   - measure strings by hand-worked cases, and the refusals.
// Prints `ok` and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "lpp_obs_string_plan.h"

using namespace lpp;
using namespace lpp::obs_host;

namespace {

struct Op {
	int op, site, spin, flag;
};

int failures = 0;
#define CHECK(cond)                                                        \
	do {                                                                   \
		if (!(cond)) {                                                     \
			std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
			failures++;                                                    \
		}                                                                  \
	} while (0)

bool plan(int conv, const std::vector<Op>& s, int L, int nup, int ndn, StringPlan& P, const char** why)
{
	std::vector<int32_t> ops, sites, spins, flags;
	for (const Op& o : s) {
		ops.push_back(o.op);
		sites.push_back(o.site);
		spins.push_back(o.spin);
		flags.push_back(o.flag);
	}
	return plan_string(conv, (int)s.size(), ops.data(), sites.data(), spins.data(), flags.data(), L, nup, ndn, P, why);
}

// destination (du, dd) -> source ranks and coefficient, as the kernels read the plan; false: not reached
bool eval(const StringPlan& P, const std::vector<uint32_t>& wu, const std::vector<uint32_t>& wd, int64_t du, int64_t dd, int64_t* su, int64_t* sd, int* coef)
{
	int32_t tu = P.tu[(size_t)du], td = P.td[(size_t)dd];
	if (tu == 0 || td == 0) return false;
	int v = ((tu < 0) != (td < 0)) ? -1 : 1;
	tu = tu < 0 ? -tu : tu;
	td = td < 0 ? -td : td;
	const uint32_t a = wu[(size_t)tu - 1], b = wd[(size_t)td - 1];
	for (int k = 0; k < P.nsz; k++) {
		const uint32_t e = P.sz[k], site = e & 31u;
		v *= (int)(((a >> site) ^ (e >> 5)) & 1u) - (int)(((b >> site) ^ (e >> 6)) & 1u);
	}
	if (v == 0) return false;
	*su = tu - 1;
	*sd = td - 1;
	*coef = v;
	return true;
}

void check_invariants(const StringPlan& P, int L, int nup, int ndn)
{
	CHECK((int64_t)P.tu.size() == binom(L, P.nup2) && (int64_t)P.td.size() == binom(L, P.ndn2));
	CHECK(P.n_up_dst == (int64_t)P.tu.size() && P.n_dn_dst == (int64_t)P.td.size());
	CHECK(P.n_up_src == binom(L, nup) && P.n_dn_src == binom(L, ndn));
	CHECK(P.nsz >= 0 && P.nsz <= kObsStringMaxOps);
	for (int sp = 0; sp < 2; sp++) {
		const std::vector<int32_t>& t = sp ? P.td : P.tu;
		const int64_t nsrc = sp ? P.n_dn_src : P.n_up_src;
		std::set<int32_t> seen;
		for (int32_t v : t) {
			if (v == 0) continue;
			const int32_t r = (v < 0 ? -v : v) - 1;
			CHECK(r >= 0 && r < nsrc);
			CHECK(seen.insert(r).second);
		}
	}
}

// the composed plan against the one-operator plans chained backwards from every destination
void check_many_point(const std::vector<Op>& s, int L, int nup, int ndn)
{
	StringPlan P;
	const char* why = nullptr;
	CHECK(plan(LPP_STRING_MANY_POINT, s, L, nup, ndn, P, &why));
	// the sector walk, one operator at a time
	std::vector<StringPlan> one(s.size());
	std::vector<std::pair<int, int>> parts { { nup, ndn } };
	bool has = true;
	for (size_t k = 0; k < s.size() && has; k++) {
		CHECK(plan(LPP_STRING_MANY_POINT, { s[k] }, L, parts.back().first, parts.back().second, one[k], &why));
		has = one[k].has;
		if (has) {
			check_invariants(one[k], L, parts.back().first, parts.back().second);
			parts.push_back({ one[k].nup2, one[k].ndn2 });
		}
	}
	CHECK(P.has == has);
	if (!P.has) return;
	check_invariants(P, L, nup, ndn);
	CHECK(P.nup2 == parts.back().first && P.ndn2 == parts.back().second && P.scale == 1.0);
	std::vector<std::vector<uint32_t>> wu(parts.size()), wd(parts.size());
	for (size_t k = 0; k < parts.size(); k++) {
		species_words(L, parts[k].first, wu[k]);
		species_words(L, parts[k].second, wd[k]);
	}
	for (int64_t dd = 0; dd < P.n_dn_dst; dd++)
		for (int64_t du = 0; du < P.n_up_dst; du++) {
			int64_t su = 0, sd = 0, cu = du, cd = dd;
			int coef = 0, chained = 1;
			const bool reached = eval(P, wu[0], wd[0], du, dd, &su, &sd, &coef);
			bool alive = true;
			for (size_t k = s.size(); k-- > 0 && alive;) {
				int c = 0;
				alive = eval(one[k], wu[k], wd[k], cu, cd, &cu, &cd, &c);
				chained *= c;
			}
			CHECK(reached == alive);
			if (reached && alive) CHECK(su == cu && sd == cd && coef == chained);
		}
}

const int C = LPP_OP_C, D = LPP_OP_CDAGGER, N = LPP_OP_N, Z = LPP_OP_SZ, P_ = LPP_OP_SPLUS, M = LPP_OP_SMINUS, I = LPP_OP_IDENTITY;
const int U = LPP_SPIN_UP, W = LPP_SPIN_DOWN;

// slot s of an image read back against the plan it came from, and the sz words against P.sz
void check_slot(const StringImage& G, const std::vector<int32_t>& img, int s, const StringPlan& P)
{
	CHECK(G.tab_dn(s) + P.td.size() <= G.words_up());
	CHECK(std::vector<int32_t>(img.begin() + (std::ptrdiff_t)G.tab_up(s), img.begin() + (std::ptrdiff_t)G.tab_dn(s)) == P.tu);
	CHECK(std::vector<int32_t>(img.begin() + (std::ptrdiff_t)G.tab_dn(s), img.begin() + (std::ptrdiff_t)(G.tab_dn(s) + P.td.size())) == P.td);
	const StringSzWords sz = pack_sz(P);
	for (int k = 0; k < kObsStringMaxOps; k++) CHECK(sz.entry(k) == (k < P.nsz ? P.sz[k] : 0));
}

// the word lists of an image against the species words of (L; nup, ndn); absent lists: nothing between the tables and the spare words
void check_words(const StringImage& G, const std::vector<int32_t>& img, int L, int nup, int ndn)
{
	CHECK(img.size() == G.size() && G.size() == (size_t)((G.ntu + G.ntd) * G.slots + G.nwu + G.nwd + 4));
	std::vector<uint32_t> wu, wd;
	if (G.nwu) species_words(L, nup, wu);
	if (G.nwd) species_words(L, ndn, wd);
	CHECK((int64_t)wu.size() == G.nwu && (int64_t)wd.size() == G.nwd);
	for (size_t i = 0; i < wu.size(); i++) CHECK((uint32_t)img[G.words_up() + i] == wu[i]);
	for (size_t i = 0; i < wd.size(); i++) CHECK((uint32_t)img[G.words_dn() + i] == wd[i]);
	for (size_t i = G.words_dn() + (size_t)G.nwd; i < img.size(); i++) CHECK(img[i] == 0);
}

// The upload images of sector (L; nup, ndn): every string alone as apply uploads it (the word lists only with sz entries), and 1, 8 and 5 of the
// strings that stay in the sector as the bracket kernel's batch of 8 slots; then the refusals.  Returns the number of strings that stay.
int check_images(const std::vector<std::vector<Op>>& strings, int L, int nup, int ndn)
{
	const char* why = nullptr;
	std::vector<StringPlan> stay;
	std::vector<int32_t> img;
	for (const auto& s : strings) {
		StringPlan P;
		CHECK(plan(LPP_STRING_MANY_POINT, s, L, nup, ndn, P, &why));
		if (!P.has) continue;
		const bool words = P.nsz > 0;
		const StringImage G { P.n_up_dst, P.n_dn_dst, 1, words ? P.n_up_src : 0, words ? P.n_dn_src : 0 };
		CHECK(string_image_begin(G, L, nup, ndn, img, &why) && string_image_tables(G, &P, 1, img, &why));
		check_slot(G, img, 0, P);
		check_words(G, img, L, nup, ndn);
		if (P.nup2 == nup && P.ndn2 == ndn) stay.push_back(P);
	}
	if (stay.empty()) return 0;
	const int64_t nu = binom(L, nup), nd = binom(L, ndn);
	const StringImage G { nu, nd, 8, nu, nd };
	CHECK(string_image_begin(G, L, nup, ndn, img, &why));
	for (int ns : { 8, 1, 5 }) { // one image reused as the driver does: a shorter batch leaves the later slots as they were
		std::vector<StringPlan> batch;
		for (int s = 0; s < ns; s++) batch.push_back(stay[(size_t)(s + ns) % stay.size()]);
		CHECK(string_image_tables(G, batch.data(), ns, img, &why));
		for (int s = 0; s < ns; s++) check_slot(G, img, s, batch[(size_t)s]);
		for (int s = ns; s < 8; s++) check_slot(G, img, s, stay[(size_t)(s + 8) % stay.size()]);
		check_words(G, img, L, nup, ndn);
	}
	// refusals: nothing is copied
	const std::vector<int32_t> before = img;
	std::vector<StringPlan> nine(9, stay[0]);
	CHECK(!string_image_tables(G, nine.data(), 9, img, &why) && why && img == before);
	std::vector<int32_t> small(img.begin(), img.end() - 1);
	CHECK(!string_image_tables(G, nine.data(), 1, small, &why));
	return (int)stay.size();
}

} // namespace

int main()
{
	const std::vector<std::vector<Op>> strings {
		{ { N, 0, U, 0 } },
		{ { Z, 1, U, 0 } },
		{ { C, 0, W, 0 } },
		{ { C, 0, U, 0 }, { D, 2, U, 0 } },
		{ { D, 1, W, 0 }, { C, 0, W, 0 } },
		{ { P_, 1, U, 0 }, { M, 3, U, 0 } },
		{ { C, 1, U, 0 }, { C, 2, W, 0 }, { D, 3, W, 0 }, { D, 0, U, 0 } },
		{ { Z, 1, U, 0 }, { C, 1, U, 0 }, { Z, 1, U, 0 }, { D, 1, U, 0 } },
		{ { M, 2, U, 0 }, { Z, 2, U, 0 }, { P_, 2, U, 0 }, { Z, 2, U, 0 }, { Z, 0, W, 0 } },
		{ { C, 0, U, 0 }, { D, 0, U, 0 } }, // through (0,0) from (1,0)
		{ { D, 0, U, 0 }, { C, 0, U, 0 } }, // leaves [0, L] from a full species
		{ { C, 0, U, 0 }, { N, 1, U, 0 }, { D, 2, W, 0 } }, // ends in another sector
		{ { C, 0, U, 0 }, { N, 3, W, 0 }, { D, 3, U, 0 }, { Z, 3, U, 0 }, { P_, 2, U, 0 }, { Z, 2, U, 0 }, { M, 2, U, 0 }, { C, 0, W, 0 }, { C, 1, W, 0 }, { N, 1, U, 0 },
		  { D, 0, W, 0 }, { Z, 0, W, 0 }, { D, 1, W, 0 }, { C, 3, U, 0 }, { D, 0, U, 0 }, { N, 0, U, 0 } }, // 16 operators
	};
	for (int L = 4; L <= 6; L++)
		for (int nup = 0; nup <= L; nup++)
			for (int ndn = 0; ndn <= L; ndn++)
				for (const auto& s : strings) check_many_point(s, L, nup, ndn);
	check_many_point(strings.back(), 12, 6, 5);
	check_many_point({ { C, 29, U, 0 }, { D, 28, U, 0 }, { Z, 29, W, 0 } }, 30, 1, 1); // the highest site

	// the largest tables the 4 x 4 cluster has: C(16, 8) entries per species
	{
		StringPlan P;
		const char* why = nullptr;
		CHECK(plan(LPP_STRING_MANY_POINT, strings.back(), 16, 8, 8, P, &why) && P.has);
		check_invariants(P, 16, 8, 8);
	}

	// the upload images: on (4; 2, 2), (5; 2, 1) with an odd sector, (6; 3, 3), and where one species has a single state
	CHECK(check_images(strings, 4, 2, 2) >= 8);
	CHECK(check_images(strings, 5, 2, 1) >= 8);
	CHECK(check_images(strings, 6, 3, 3) >= 8);
	CHECK(check_images(strings, 4, 4, 1) >= 1);
	// A plan whose table length is not the image's species count is REFUSED by the packer, each species on its own, and nothing is copied:
	// c up ends in (1, 2), so its up table has C(4, 1) = 4 entries where the image of (2, 2) has slots of C(4, 2) = 6; c down likewise
	{
		const StringImage G { 6, 6, 8, 6, 6 };
		std::vector<int32_t> img;
		const char* why = nullptr;
		CHECK(string_image_begin(G, 4, 2, 2, img, &why));
		const std::vector<int32_t> before = img;
		StringPlan ok, up, dn;
		CHECK(plan(LPP_STRING_MANY_POINT, { { N, 0, U, 0 } }, 4, 2, 2, ok, &why) && ok.tu.size() == 6 && ok.td.size() == 6);
		CHECK(plan(LPP_STRING_MANY_POINT, { { C, 0, U, 0 } }, 4, 2, 2, up, &why) && up.has && up.tu.size() == 4 && up.td.size() == 6);
		CHECK(plan(LPP_STRING_MANY_POINT, { { C, 0, W, 0 } }, 4, 2, 2, dn, &why) && dn.has && dn.tu.size() == 6 && dn.td.size() == 4);
		for (const StringPlan& bad : { up, dn }) {
			const std::vector<StringPlan> batch { ok, bad };
			why = nullptr;
			CHECK(!string_image_tables(G, batch.data(), 2, img, &why) && why && img == before); // the good plan before it is not copied either
		}
		StringPlan grown = ok; // one entry too many: it would run into the next slot
		grown.tu.push_back(0);
		CHECK(!string_image_tables(G, &grown, 1, img, &why) && img == before);
		// the word lists of another sector are refused as well
		CHECK(!string_image_begin(G, 4, 1, 2, img, &why) && !string_image_begin(G, 4, 2, 3, img, &why));
	}

	// measure: hand-worked cases on L = 3, sector (1, 1): up words 1, 2, 4 by rank
	{
		StringPlan P;
		const char* why = nullptr;
		CHECK(plan(LPP_STRING_MEASURE, { { N, 1, U, 0 } }, 3, 1, 1, P, &why) && P.has);
		CHECK(P.tu == (std::vector<int32_t> { 0, 2, 0 }) && P.td == (std::vector<int32_t> { 1, 2, 3 }) && P.scale == 1.0 && P.nsz == 0);
		CHECK(plan(LPP_STRING_MEASURE, { { Z, 1, W, 0 }, { I, 0, U, 0 } }, 3, 1, 1, P, &why) && P.has);
		CHECK(P.td == (std::vector<int32_t> { 1, -2, 3 }) && P.scale == 0.5);
		// c'[2] c[0] on the up word 001 -> 100, no electron in between: +1; the LAST listed acts first
		CHECK(plan(LPP_STRING_MEASURE, { { C, 2, U, 1 }, { C, 0, U, 0 } }, 3, 1, 1, P, &why) && P.has);
		CHECK(P.tu == (std::vector<int32_t> { 0, 0, 1 }));
		// the same for the down species: one up electron is passed twice, +1
		CHECK(plan(LPP_STRING_MEASURE, { { C, 2, W, 1 }, { C, 0, W, 0 } }, 3, 1, 1, P, &why) && P.has);
		CHECK(P.td == (std::vector<int32_t> { 0, 0, 1 }));
		// an up electron created between the two down operators: the down string sees 1 up electron, then 2: -1
		CHECK(plan(LPP_STRING_MEASURE, { { C, 1, U, 0 }, { C, 2, W, 1 }, { C, 1, U, 1 }, { C, 0, W, 0 } }, 3, 0, 1, P, &why) && P.has);
		CHECK(P.td == (std::vector<int32_t> { 0, 0, -1 }) && P.tu == (std::vector<int32_t> { 1 }));
		// conserving but dead: c on an empty species first
		CHECK(plan(LPP_STRING_MEASURE, { { C, 0, U, 1 }, { C, 0, U, 0 } }, 3, 0, 1, P, &why) && P.has && P.tu == (std::vector<int32_t> { 0 }));
		check_invariants(P, 3, 0, 1);
	}

	// refusals
	{
		StringPlan P;
		const char* why = nullptr;
		CHECK(!plan(LPP_STRING_MEASURE, { { C, 0, U, 0 } }, 4, 2, 2, P, &why) && why);
		CHECK(!plan(LPP_STRING_MEASURE, { { C, 0, U, 1 }, { C, 0, W, 0 } }, 4, 2, 2, P, &why));
		CHECK(!plan(LPP_STRING_MEASURE, { { P_, 0, U, 0 } }, 4, 2, 2, P, &why));
		CHECK(!plan(LPP_STRING_MANY_POINT, { { I, 0, U, 0 } }, 4, 2, 2, P, &why));
		CHECK(!plan(LPP_STRING_MANY_POINT, { { N, 4, U, 0 } }, 4, 2, 2, P, &why));
		CHECK(!plan(LPP_STRING_MANY_POINT, { { N, -1, U, 0 } }, 4, 2, 2, P, &why));
		CHECK(!plan(LPP_STRING_MANY_POINT, { { N, 0, 2, 0 } }, 4, 2, 2, P, &why));
		CHECK(!plan(LPP_STRING_MANY_POINT, { { N, 0, U, 0 } }, 4, 5, 2, P, &why));
		CHECK(!plan(LPP_STRING_MANY_POINT, { { N, 0, U, 0 } }, 31, 1, 1, P, &why));
		CHECK(!plan(2, { { N, 0, U, 0 } }, 4, 2, 2, P, &why));
		CHECK(!plan(LPP_STRING_MANY_POINT, std::vector<Op>(17, Op { N, 0, U, 0 }), 4, 2, 2, P, &why));
		CHECK(!plan(LPP_STRING_MANY_POINT, {}, 4, 2, 2, P, &why));
	}
	if (failures) return 1;
	std::printf("ok\n");
	return 0;
}
