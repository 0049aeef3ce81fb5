// cgck_pcb_plan.cpp — cgck_pcb_table_bytes (no device, no context): the bytes of
// cgck_pcb_build's table as a pure function of nconn.  8 bytes for each of
// pcb_slots(nconn) slots (cgck_pcb_probe.h): the power of two at or above
// 2 nconn, at least 2.  The 4-byte shape of the A/B uses the first half.
#include "cgck_pcb_probe.h"

extern "C" size_t cgck_pcb_table_bytes(uint32_t nconn)
{
	return nconn > cgck::kPcbMaxConn ? 0 : (size_t)cgck::pcb_slots(nconn) * 8;
}
