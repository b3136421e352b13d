// lpp_txgeom.h -- the geometry of the transposition exchange, described once.  Host-only and self-contained (no HIP, nothing to link):
// the engine's set-up entry points (lpp_assemble.hip) and a stand-alone host program (tests/host/tx_geometry_main.cpp) include it.
#pragma once
#include <stdint.h>

#include "../../include/lpp_engine.h"

namespace lpp {

// The transposition exchange (multi-GPU Hubbard, include/lpp_engine.h): a rank owns `per` down configurations and, of the
// transposed slice, `peru` up indices; xchg_chunk = per * peru.  Described once; what a bad geometry means is the caller's policy
// ("Matrix set-up entry points").
struct TxGeom {
	int64_t per = 0, peru = 0; // ceil(N_down / P); xchg_chunk / per
	bool requested = false; // the communicator carries the exchange: both callbacks and xchg_chunk > 0
	bool valid = false; // ... and send2 / recv2 are there, xchg_chunk == per * peru, peru * P >= N_up
	bool mult16 = false; // peru is a multiple of 16: the product-basis kernels can serve the transposed slice
	bool fits32 = false; // the transposed slice, P * per * peru elements, stays within 32-bit column indices
	const char* reason = ""; // !valid: what is missing
};
// what a caller that fails on !valid says after its own prefix
constexpr const char* kTxGeomNeeds = "transposition exchange needs send2/recv2 buffers and xchg_chunk == ceil(N_down/P) * peru, peru >= ceil(N_up/P)";
inline TxGeom tx_geometry(const lpp_comm* comm, int64_t n_up, int64_t n_dn)
{
	TxGeom g;
	const int64_t P = comm && comm->nranks > 0 ? comm->nranks : 1;
	g.per = (n_dn + P - 1) / P;
	g.requested = comm && comm->exchange_begin && comm->exchange_end && comm->xchg_chunk > 0;
	if (!g.requested) {
		g.reason = "no transposition exchange in the communicator";
		return g;
	}
	g.peru = g.per > 0 ? comm->xchg_chunk / g.per : 0;
	g.mult16 = (g.peru & 15) == 0;
	g.fits32 = P * g.per * g.peru <= (int64_t)INT32_MAX;
	if (!comm->send2_buf || !comm->recv2_buf)
		g.reason = "send2 / recv2 buffers missing";
	else if (g.per <= 0 || comm->xchg_chunk != g.per * g.peru)
		g.reason = "xchg_chunk is not a multiple of ceil(N_down/P)";
	else if (g.peru * P < n_up)
		g.reason = "peru * P < N_up";
	else
		g.valid = true;
	return g;
}

} // namespace lpp
