// arp_host.cpp — libarpeggio_host.so: the host-only entry points of include/arpeggio_hip.h built with g++ (no HIP, no GPU):
// the mmCIF category reader (arp_cif_*), the JSON writer of the atom-atom records (arp_write_contacts_json) and the placement
// of a batch's structures in their common grid (arp_batch_layout).  The same sources as in libarpeggio_hip.so (arp_cif.h,
// arp_cif_api.h, arp_json.h, arp_batchgrid.h); arpeggio_amd/_capi.py falls back to this library
// for these calls when the HIP library has not been built (a checkout on a machine without hipcc: tests/golden/make_golden*.py).
#include <cstdint>
#include <cstring>

#include "../../include/arpeggio_hip.h"
#include "arp_batchgrid.h"
#include "arp_cif.h"
#include "arp_json.h"

extern "C" const char* arp_host_version(void) { return "arpeggio_host 0.2.0 (host-only subset: arp_cif_*, arp_write_contacts_json, arp_batch_layout)"; }
#include "arp_cif_api.h"      // (C linkage from the prototypes of the public header)

extern "C" int arp_batch_layout(int64_t nstruct, const double* boxes, double radius, int32_t* places_out, int32_t dims_out[3], double* edge_out) {
    return batch_layout_c(nstruct, boxes, radius, places_out, dims_out, edge_out) == 0 ? ARP_OK : ARP_E_ARG;
}
