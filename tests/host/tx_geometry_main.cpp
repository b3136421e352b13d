// tx_geometry_main.cpp -- prints lpp::tx_geometry (csrc/lpp_txgeom.h) for "n_up n_dn nranks xchg_chunk" quadruples given as arguments:
// a host-only program (tests/test_tx_geometry.py builds it with the address and undefined-behaviour sanitizers).
#include <cstdio>
#include <cstdlib>

#include "lpp_txgeom.h"

static int32_t xchg(void*, int32_t) { return 0; }

int main(int argc, char** argv)
{
	static double buf[2];
	for (int a = 1; a + 3 < argc; a += 4) {
		const int64_t n_up = atoll(argv[a]), n_dn = atoll(argv[a + 1]);
		lpp_comm c {};
		c.nranks = atoi(argv[a + 2]);
		c.xchg_chunk = atoll(argv[a + 3]);
		c.send2_buf = &buf[0];
		c.recv2_buf = &buf[1];
		c.exchange_begin = c.exchange_end = xchg;
		const lpp::TxGeom g = lpp::tx_geometry(&c, n_up, n_dn);
		printf("%lld %lld %d %lld: per=%lld peru=%lld requested=%d valid=%d mult16=%d fits32=%d reason=%s\n", (long long)n_up, (long long)n_dn, (int)c.nranks,
		       (long long)c.xchg_chunk, (long long)g.per, (long long)g.peru, (int)g.requested, (int)g.valid, (int)g.mult16, (int)g.fits32, g.reason);
	}
	return 0;
}
