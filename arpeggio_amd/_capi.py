"""ctypes binding of include/arpeggio_hip.h (libarpeggio_hip.so).

There is no CPU fallback: if the library is missing or no GPU is usable the calls
raise NativeLibraryError.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import tables
from .core.exceptions import NativeLibraryError

_HERE = os.path.dirname(os.path.abspath(__file__))
# ARP_LIB_PATH: another build of the same library (A/B comparisons of kernel variants on one GPU box)
LIB_PATH = os.environ.get('ARP_LIB_PATH') or os.path.join(_HERE, 'csrc', 'libarpeggio_hip.so')

ARP_OK, ARP_E_ARG, ARP_E_HIP, ARP_E_CAPACITY, ARP_E_XBOND_NBR, ARP_E_NOMEM = 0, -1, -2, -3, -4, -5

# every symbol declared in include/arpeggio_hip.h
SYMBOLS = (
    'arp_version', 'arp_create', 'arp_destroy', 'arp_last_error', 'arp_set_atoms', 'arp_set_residues',
    'arp_set_bonds', 'arp_set_hydrogens', 'arp_set_single_bond_neighbours', 'arp_set_rings', 'arp_set_amides',
    'arp_search_all', 'arp_search', 'arp_make_selection', 'arp_atom_contacts_launch', 'arp_atom_contacts_fetch',
    'arp_atom_contacts', 'arp_atom_plane', 'arp_plane_plane', 'arp_group_group', 'arp_group_plane',
    'arp_set_ownership', 'arp_get_stats', 'arp_set_profiling', 'arp_get_kernel_times', 'arp_stream_handle',
    'arp_set_selection', 'arp_run_launch', 'arp_run_enqueue', 'arp_run_wait', 'arp_atom_plane_launch', 'arp_plane_plane_launch', 'arp_group_group_launch',
    'arp_group_plane_launch', 'arp_atom_plane_fetch', 'arp_plane_plane_fetch', 'arp_group_group_fetch',
    'arp_group_plane_fetch', 'arp_get_selection', 'arp_set_group_ownership', 'arp_set_single_bond_neighbour_coords',
    'arp_set_selection_state', 'arp_atom_accumulators', 'arp_device_buffer', 'arp_run_stage', 'arp_use_stream',
    'arp_get_host_times', 'arp_set_whole_structure', 'arp_set_grid_reuse', 'arp_set_sort_after_pass', 'arp_set_packed_layout', 'arp_set_batch', 'arp_device_count', 'arp_device_synchronize', 'arp_comm_unique_id', 'arp_comm_init', 'arp_comm_destroy', 'arp_comm_info',
    'arp_shard_exchange_faces', 'arp_shard_set_exchange_lists', 'arp_shard_exchange_plus', 'arp_shard_reduce_residue_sets', 'arp_ring_geometry', 'arp_amide_geometry', 'arp_ring_residues',
    'arp_host_alloc', 'arp_host_free', 'arp_atom_integer_sifts', 'arp_blob_size', 'arp_blob_layout', 'arp_set_blob', 'arp_blob_fill',
    'arp_write_contacts_json', 'arp_records_size', 'arp_records_layout', 'arp_records_fill', 'arp_shard_set_home', 'arp_shard_pack_face',
    'arp_shard_assemble', 'arp_shard_layout', 'arp_get_blob', 'arp_cif_open', 'arp_cif_close', 'arp_cif_rows', 'arp_cif_cols',
    'arp_cif_blocks', 'arp_cif_tag', 'arp_cif_text', 'arp_cif_column', 'arp_cif_column_f64', 'arp_cif_column_i64',
    'arp_atom_contacts_sort', 'arp_fetch_packed', 'arp_set_topology', 'arp_set_models', 'arp_models_planes',
    'arp_models_persistence_launch', 'arp_models_persistence_fetch', 'arp_set_compact_lookback',
    'arp_residue_pairs_launch', 'arp_residue_pairs_fetch',
    'arp_models_residue_persistence_launch', 'arp_models_residue_persistence_fetch',
    'arp_contacts_filter_launch', 'arp_fetch_packed_filtered',
    'arp_water_bridges_launch', 'arp_water_bridges_fetch',
    'arp_models_water_bridge_persistence_launch', 'arp_models_water_bridge_persistence_fetch',
    'arp_batch_layout',
    'arp_models_similarity_launch', 'arp_models_similarity_fetch', 'arp_models_similarity_info',
    'arp_models_coupling_launch', 'arp_models_coupling_fetch', 'arp_models_coupling_info',
    'arp_models_lifetimes_launch', 'arp_models_lifetimes_fetch', 'arp_models_lifetimes_info',
    'arp_networks_launch', 'arp_networks_fetch', 'arp_networks_labels_fetch', 'arp_networks_info',
    'arp_poses_contacts_launch', 'arp_poses_contacts_fetch', 'arp_poses_contacts_info',
    'arp_set_plane_atoms', 'arp_poses_planes_launch', 'arp_poses_planes_fetch', 'arp_poses_planes_info',
    'arp_poses_fingerprints_launch', 'arp_poses_fingerprints_fetch', 'arp_poses_fingerprints_info',
    'arp_poses_fingerprints_planes_launch',
    'arp_poses_shortlist_launch', 'arp_poses_shortlist_fetch', 'arp_poses_shortlist_planes_fetch', 'arp_poses_shortlist_info',
    'arp_poses_clusters_launch', 'arp_poses_clusters_fetch', 'arp_poses_clusters_info',
    'arp_set_ligand_library', 'arp_library_contacts_launch', 'arp_library_contacts_fetch', 'arp_library_info',
    'arp_library_best_launch', 'arp_library_best_fetch',
    'arp_library_fingerprints_launch', 'arp_library_fingerprints_fetch', 'arp_library_fingerprints_info',
    'arp_library_fingerprints_best_launch', 'arp_library_fingerprints_best_fetch',
    'arp_library_fingerprints_planes_launch',
    'arp_set_ligand_library_planes', 'arp_library_planes_launch', 'arp_library_planes_fetch', 'arp_library_planes_info',
    'arp_library_shortlist_launch', 'arp_library_shortlist_fetch', 'arp_library_shortlist_planes_fetch', 'arp_library_shortlist_info',
    'arp_library_clusters_launch', 'arp_library_clusters_fetch', 'arp_library_clusters_info',
    'arp_library_water_bridges_launch', 'arp_library_water_bridges_fetch', 'arp_library_water_bridges_info',
)

# the three device-reduced tables (tables.py holds their columns, in the order of their fetch's arguments) and ARP_PERSIST_STAGE_MAX
PERSIST_BITS = RESPAIR_BITS = RESPERSIST_BITS = WBP_BITS = tables.N_BITS
# ligand poses on the resident receptor (ARP_POSES_*)
POSES_MAX_ATOMS, POSES_MAX_POSES, POSES_MAX_CUTOFF, POSES_SUMMARY = 1024, 1 << 20, 6.0, 16
# ... their ring and amide contacts (ARP_POSES_PLANES_*)
POSES_PLANES_SUMMARY, POSES_PLANES_MAX_RINGS, POSES_PLANES_MAX_HOME, POSES_PLANES_MAX_AMIDES, POSES_PLANES_MAX_NEAR = 16, 512, 512, 512, 256
# ... their fingerprints (ARP_POSEFP_*)
POSEFP_PLANES, POSEFP_MAX_REFS, POSEFP_BY_RESIDUE, POSEFP_ALL_PAIRS = 15, 64, 1, 2
POSEFP_ALL_PLANES = 29           # ARP_POSEFP_ALL_PLANES: the SIFt bits and the 14 ring / amide class planes behind them
# ... their shortlist (ARP_SHORTLIST_*)
SHORTLIST_LIST, SHORTLIST_SUMMARY, SHORTLIST_TANIMOTO, SHORTLIST_TABLES, SHORTLIST_MAX_WEIGHT = 0, 1, 2, 5, 1 << 24
INT64_MIN = -(1 << 63)
LIBRARY_SHORTLIST_POSES, LIBRARY_SHORTLIST_LIGANDS = 0, 1      # ARP_LIBRARY_SHORTLIST_*
# a ligand library on the resident receptor (ARP_LIBRARY_*)
LIBRARY_MAX_LIGANDS, LIBRARY_MAX_ATOMS = 1 << 16, 256
LIBFP_MAX_FEATURES = 1 << 22     # ARP_LIBFP_MAX_FEATURES: reference features of a library fingerprint launch
# ... their clusters (ARP_POSECL_*; the rounds enqueued between two waits of arp_poses_clusters_launch)
POSECL_MAX_CLUSTERS, POSECL_ROUNDS_PER_WAIT = 4096, 64
# ... the clusters of a library (ARP_LIBCL_*; the rounds enqueued between two waits of arp_library_clusters_launch)
LIBCL_ALL, LIBCL_LIST, LIBCL_SHORTLIST, LIBCL_WINDOW, LIBCL_LDS_WORDS, LIBCL_ROUNDS_PER_WAIT = 0, 1, 2, 32, 2048, 32
WBP_BY_RESIDUE = 1 << 1          # ARP_WBP_BY_RESIDUE (beside water_bridges.SAME_RESIDUE, ARP_WB_SAME_RESIDUE)
PERSIST_STAGE_MAX = 0
SIM_PLANES, SIM_MAX_MODELS, SIM_BY_RESIDUE = 20, 4096, 1      # ARP_SIM_PLANES, ARP_SIM_MAX_MODELS, ARP_SIM_BY_RESIDUE
COUPLE_BY_RESIDUE, COUPLE_MAX_FEATURES = 1, 65536              # ARP_COUPLE_BY_RESIDUE, ARP_COUPLE_MAX_FEATURES
CTYPE_ALL = 0x7F                 # ARP_FILTER_CTYPE_ALL
LIFETIMES_MAX_GAP = 65534        # ARP_LIFETIMES_MAX_GAP
NET_BY_RESIDUE = 1               # ARP_NET_BY_RESIDUE
PERSIST_COLUMNS, RESPAIR_COLUMNS, RESPERSIST_COLUMNS = tables.PERSIST.columns, tables.RESPAIR.columns, tables.RESPERSIST.columns

_lib = None


def device_count():
    """GPUs this process can see (the library's own answer: no torch involved)."""
    return int(load().arp_device_count())


def _declare_host_entry_points(L):
    """argtypes of the host-only entry points (mmCIF reader, JSON writer, batch layout): the same in both libraries."""
    vp, i64, dbl, i32 = C.c_void_p, C.c_int64, C.c_double, C.c_int
    L.arp_batch_layout.argtypes = [i64, vp, dbl, vp, vp, C.POINTER(dbl)]
    L.arp_batch_layout.restype = C.c_int
    L.arp_cif_open.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.POINTER(vp), C.c_char_p, C.c_uint64]
    L.arp_cif_close.argtypes = [vp]
    L.arp_cif_close.restype = None
    L.arp_cif_rows.argtypes = [vp]
    L.arp_cif_rows.restype = C.c_int64
    L.arp_cif_cols.argtypes = [vp]
    L.arp_cif_blocks.argtypes = [vp]
    L.arp_cif_tag.argtypes = [vp, i32]
    L.arp_cif_tag.restype = C.c_char_p
    L.arp_cif_text.argtypes = [vp]
    L.arp_cif_text.restype = vp
    L.arp_cif_column.argtypes = [vp, i32, vp, vp, vp]
    L.arp_cif_column_f64.argtypes = [vp, i32, dbl, vp, C.POINTER(i64)]
    L.arp_cif_column_i64.argtypes = [vp, i32, i64, vp, C.POINTER(i64)]
    L.arp_write_contacts_json.argtypes = [C.c_char_p, i32, i32, i64, vp, vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, C.c_char_p, i64]


HOST_LIB_PATH = os.path.join(_HERE, 'csrc', 'libarpeggio_host.so')
HOST_SYMBOLS = ('arp_cif_open', 'arp_cif_close', 'arp_cif_rows', 'arp_cif_cols', 'arp_cif_blocks', 'arp_cif_tag', 'arp_cif_text', 'arp_cif_column',
                'arp_cif_column_f64', 'arp_cif_column_i64', 'arp_write_contacts_json', 'arp_batch_layout')
_host_lib = None


def load_host():
    """The library for the HOST-ONLY entry points (the mmCIF category reader, the JSON writer of the records): the HIP library
    when it has been built — it holds them too —, otherwise ``libarpeggio_host.so``, the same sources (csrc/arp_cif.h,
    arp_cif_api.h, arp_json.h) compiled with g++ (``arpeggio_amd.build.build_host``; built on first use).  No compute entry
    point lives there: a machine without hipcc can read files and regenerate the golden fixtures, nothing more."""
    global _host_lib
    if _lib is not None:
        return _lib
    if _host_lib is not None:
        return _host_lib
    if os.path.exists(LIB_PATH):
        return load()
    from . import build as _build
    path = _build.build_host()
    try:
        L = C.CDLL(path)
    except OSError as e:
        raise NativeLibraryError(f'cannot load {path}: {e}') from e
    _declare_host_entry_points(L)
    _host_lib = L
    return L


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(f'{LIB_PATH} not found: build it with `python -m arpeggio_amd.build` '
                                 '(hipcc --offload-arch=gfx950); there is no CPU fallback')
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:
        raise NativeLibraryError(f'cannot load {LIB_PATH}: {e}') from e
    vp, i64, dbl, i32 = C.c_void_p, C.c_int64, C.c_double, C.c_int
    L.arp_version.restype = C.c_char_p
    L.arp_last_error.restype = C.c_char_p
    L.arp_last_error.argtypes = [vp]
    L.arp_create.argtypes = [i32, C.POINTER(vp)]
    L.arp_destroy.argtypes = [vp]
    L.arp_destroy.restype = None
    L.arp_set_atoms.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp]
    L.arp_set_residues.argtypes = [vp, i64, vp, vp, vp]
    L.arp_set_bonds.argtypes = [vp, vp, vp]
    L.arp_set_hydrogens.argtypes = [vp, vp, vp]
    L.arp_set_single_bond_neighbours.argtypes = [vp, vp]
    L.arp_set_rings.argtypes = [vp, i64, vp, vp, vp]
    L.arp_set_amides.argtypes = [vp, i64, vp, vp, vp]
    L.arp_search_all.argtypes = [vp, dbl, vp, i64, vp, vp, C.POINTER(i64)]
    L.arp_search.argtypes = [vp, dbl, i64, vp, i64, vp, vp, C.POINTER(i64)]
    L.arp_make_selection.argtypes = [vp, vp, dbl, vp, vp, vp, vp, vp]
    L.arp_atom_contacts_launch.argtypes = [vp, dbl, dbl, i32, C.POINTER(i64)]
    L.arp_atom_contacts_fetch.argtypes = [vp, i64, vp, vp, vp, vp, vp, C.POINTER(i64)]
    L.arp_atom_contacts.argtypes = [vp, dbl, dbl, i32, i64, vp, vp, vp, vp, vp, C.POINTER(i64)]
    L.arp_atom_contacts_sort.argtypes = [vp]
    L.arp_fetch_packed.argtypes = [vp, vp, C.c_uint64, vp, vp, C.POINTER(C.c_uint64)]
    for name in tables.PLANE_BAGS:      # launch + fetch, and fetch alone: cap, one pointer per column, count
        for fn in (getattr(L, f'arp_{name}'), getattr(L, f'arp_{name}_fetch')):
            fn.argtypes = [vp, i64] + [vp] * len(tables.bag_columns(name)) + [C.POINTER(i64)]
    L.arp_set_ownership.argtypes = [vp, vp, vp]
    L.arp_set_selection.argtypes = [vp, vp]
    L.arp_atom_accumulators.argtypes = [vp, vp, vp]
    L.arp_atom_integer_sifts.argtypes = [vp, vp]
    L.arp_blob_size.argtypes = [i64] * 6
    L.arp_blob_size.restype = C.c_uint64
    L.arp_blob_layout.argtypes = [vp, C.c_uint64] + [i64] * 6
    L.arp_set_blob.argtypes = [vp, vp, C.c_uint64]
    L.arp_blob_fill.argtypes = [vp, C.c_uint64] + [vp] * 20
    L.arp_records_size.argtypes = [i64] * 5
    L.arp_records_size.restype = C.c_uint64
    L.arp_records_layout.argtypes = [vp, C.c_uint64] + [i64] * 5
    L.arp_records_fill.argtypes = [vp, C.c_uint64, i64, i64, i64, i64] + [vp] * 24
    L.arp_shard_set_home.argtypes = [vp, vp, C.c_uint64]
    L.arp_shard_pack_face.argtypes = [vp, i32, dbl, dbl, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.arp_shard_assemble.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, i64, vp]
    L.arp_shard_layout.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.arp_get_blob.argtypes = [vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    _declare_host_entry_points(L)
    L.arp_device_buffer.argtypes = [vp, i32, C.POINTER(C.c_uint64), C.POINTER(i64)]
    L.arp_run_stage.argtypes = [vp, i32, dbl, dbl, i32, dbl, vp]
    L.arp_set_group_ownership.argtypes = [vp, vp, vp, vp, vp]
    L.arp_set_single_bond_neighbour_coords.argtypes = [vp, vp, vp]
    L.arp_set_selection_state.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.arp_get_selection.argtypes = [vp, vp, vp, vp, vp, vp]
    L.arp_run_launch.argtypes = [vp, dbl, dbl, i32, dbl, vp]
    L.arp_run_enqueue.argtypes = [vp, dbl, dbl, i32, dbl]
    L.arp_run_wait.argtypes = [vp, vp]
    for nm in ('atom_plane', 'plane_plane', 'group_group', 'group_plane'):
        getattr(L, f'arp_{nm}_launch').argtypes = [vp, C.POINTER(i64)]
        getattr(L, f'arp_{nm}_fetch').argtypes = getattr(L, f'arp_{nm}').argtypes
    L.arp_get_stats.argtypes = [vp, vp]
    L.arp_set_profiling.argtypes = [vp, i32]
    L.arp_get_kernel_times.argtypes = [vp, vp, vp, i32]
    L.arp_get_host_times.argtypes = [vp, vp, vp, i32]
    L.arp_set_whole_structure.argtypes = [vp, i32]
    L.arp_set_grid_reuse.argtypes = [vp, i32]
    L.arp_set_compact_lookback.argtypes = [vp, i32]
    L.arp_set_sort_after_pass.argtypes = [vp, i32]
    L.arp_set_packed_layout.argtypes = [vp, i32]
    L.arp_device_synchronize.argtypes = [vp]
    L.arp_set_batch.argtypes = [vp, i64, vp, vp, vp, vp]
    L.arp_set_topology.argtypes = [vp, vp, C.c_uint64, vp, vp, vp]
    L.arp_set_models.argtypes = [vp, i64, vp, vp]
    L.arp_models_planes.argtypes = [vp, vp, vp, vp, vp, vp]
    L.arp_models_persistence_launch.argtypes = [vp, C.POINTER(i64)]
    L.arp_models_persistence_fetch.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64)]
    L.arp_residue_pairs_launch.argtypes = [vp, C.POINTER(i64)]
    L.arp_residue_pairs_fetch.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64)]
    L.arp_models_residue_persistence_launch.argtypes = [vp, C.POINTER(i64)]
    L.arp_models_residue_persistence_fetch.argtypes = [vp, i64] + [vp] * 12 + [C.POINTER(i64)]
    L.arp_contacts_filter_launch.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(i64)]
    L.arp_fetch_packed_filtered.argtypes = L.arp_fetch_packed.argtypes
    L.arp_water_bridges_launch.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(i64)]
    L.arp_water_bridges_fetch.argtypes = [vp, i64] + [vp] * 9 + [C.POINTER(i64)]
    L.arp_models_water_bridge_persistence_launch.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(i64)]
    L.arp_models_water_bridge_persistence_fetch.argtypes = [vp, i64] + [vp] * 14 + [C.POINTER(i64)]
    L.arp_models_similarity_launch.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(i64), C.POINTER(i64)]
    L.arp_models_similarity_fetch.argtypes = [vp, i64, vp, C.POINTER(i64)]
    L.arp_models_similarity_info.argtypes = [vp, vp]
    L.arp_models_coupling_launch.argtypes = [vp] + [C.c_uint32] * 6 + [i64, C.POINTER(i64), C.POINTER(i64)]
    L.arp_models_coupling_fetch.argtypes = [vp, i64, i64] + [vp] * 6 + [C.POINTER(i64), C.POINTER(i64)]
    L.arp_models_coupling_info.argtypes = [vp, vp]
    L.arp_models_lifetimes_launch.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(i64)]
    L.arp_models_lifetimes_fetch.argtypes = [vp, i64] + [vp] * 11 + [C.POINTER(i64)]
    L.arp_models_lifetimes_info.argtypes = [vp, vp]
    L.arp_networks_launch.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(i64)]
    L.arp_networks_fetch.argtypes = [vp, i64] + [vp] * 5 + [C.POINTER(i64)]
    L.arp_networks_labels_fetch.argtypes = [vp, i64, vp, C.POINTER(i64)]
    L.arp_networks_info.argtypes = [vp, vp]
    L.arp_poses_contacts_launch.argtypes = [vp, i64, vp, vp, C.c_double, C.c_double, C.c_int, C.POINTER(i64)]
    L.arp_poses_contacts_fetch.argtypes = [vp, i64] + [vp] * 7 + [C.POINTER(i64)]
    L.arp_poses_contacts_info.argtypes = [vp, vp]
    L.arp_set_plane_atoms.argtypes = [vp, vp, vp, vp]
    L.arp_poses_planes_launch.argtypes = [vp, i64, vp, vp]
    L.arp_poses_planes_fetch.argtypes = [vp, C.c_int, i64] + [vp] * 11 + [C.POINTER(i64)]
    L.arp_poses_planes_info.argtypes = [vp, vp]
    L.arp_poses_fingerprints_launch.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, i64, vp]
    L.arp_poses_fingerprints_planes_launch.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, i64, vp]
    L.arp_poses_fingerprints_fetch.argtypes = [vp, i64] + [vp] * 6 + [C.POINTER(i64)]
    L.arp_poses_fingerprints_info.argtypes = [vp, vp]
    L.arp_poses_shortlist_launch.argtypes = [vp, C.c_int, vp, i64, vp, i64, i64, i64, i64, C.c_uint32, C.c_uint32, C.c_uint32, vp]
    L.arp_poses_shortlist_fetch.argtypes = [vp, i64, i64] + [vp] * 10 + [C.POINTER(i64), C.POINTER(i64)]
    L.arp_poses_shortlist_planes_fetch.argtypes = [vp, C.c_int, i64, i64] + [vp] * 10 + [C.POINTER(i64)]
    L.arp_poses_shortlist_info.argtypes = [vp, vp]
    L.arp_library_shortlist_launch.argtypes = [vp, C.c_int, C.c_int, vp, i64, vp, i64, i64, i64, C.c_uint32, C.c_uint32, C.c_uint32, vp]
    L.arp_library_shortlist_fetch.argtypes = [vp, i64, i64] + [vp] * 11 + [C.POINTER(i64), C.POINTER(i64)]
    L.arp_library_shortlist_planes_fetch.argtypes = [vp, C.c_int, i64, i64] + [vp] * 10 + [C.POINTER(i64)]
    L.arp_library_shortlist_info.argtypes = [vp, vp]
    L.arp_poses_clusters_launch.argtypes = [vp, vp, i64, i64, C.c_uint64, i64, vp]
    L.arp_poses_clusters_fetch.argtypes = [vp, i64, i64] + [vp] * 6 + [C.POINTER(i64), C.POINTER(i64)]
    L.arp_poses_clusters_info.argtypes = [vp, vp]
    L.arp_library_clusters_launch.argtypes = [vp, C.c_int, vp, i64, C.c_uint64, i64, vp]
    L.arp_library_clusters_fetch.argtypes = [vp, i64, i64] + [vp] * 7 + [C.POINTER(i64), C.POINTER(i64)]
    L.arp_library_clusters_info.argtypes = [vp, vp]
    L.arp_library_water_bridges_launch.argtypes = [vp, C.c_uint32, C.POINTER(i64)]
    L.arp_library_water_bridges_fetch.argtypes = [vp, i64, i64] + [vp] * 11 + [C.POINTER(i64)]
    L.arp_library_water_bridges_info.argtypes = [vp, vp]
    L.arp_set_ligand_library.argtypes = [vp, i64] + [vp] * 7
    L.arp_library_contacts_launch.argtypes = [vp, vp, vp, vp, C.c_double, C.c_double, C.c_int, C.POINTER(i64)]
    L.arp_library_contacts_fetch.argtypes = [vp, i64] + [vp] * 7 + [C.POINTER(i64)]
    L.arp_library_info.argtypes = [vp, vp]
    L.arp_library_best_launch.argtypes = [vp, vp]
    L.arp_library_best_fetch.argtypes = [vp, i64, vp, vp, vp, C.POINTER(i64)]
    L.arp_library_fingerprints_launch.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, i64, vp, vp, vp, vp]
    L.arp_library_fingerprints_planes_launch.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, i64, vp, vp, vp, vp]
    L.arp_library_fingerprints_fetch.argtypes = [vp, i64] + [vp] * 5 + [C.POINTER(i64)]
    L.arp_library_fingerprints_info.argtypes = [vp, vp]
    L.arp_library_fingerprints_best_launch.argtypes = [vp]
    L.arp_library_fingerprints_best_fetch.argtypes = [vp, i64] + [vp] * 5 + [C.POINTER(i64), C.POINTER(i64)]
    L.arp_set_ligand_library_planes.argtypes = [vp] * 6
    L.arp_library_planes_launch.argtypes = [vp, vp, vp, vp]
    L.arp_library_planes_fetch.argtypes = [vp, C.c_int, i64] + [vp] * 11 + [C.POINTER(i64)]
    L.arp_library_planes_info.argtypes = [vp, vp]
    L.arp_comm_unique_id.argtypes = [vp, C.c_uint64]
    L.arp_comm_init.argtypes = [vp, i32, i32, vp]
    L.arp_comm_destroy.argtypes = [vp]
    L.arp_comm_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.arp_shard_exchange_faces.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, vp]
    L.arp_shard_set_exchange_lists.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, i64]
    L.arp_shard_exchange_plus.argtypes = [vp]
    L.arp_shard_reduce_residue_sets.argtypes = [vp]
    L.arp_ring_geometry.argtypes = [vp, i64, vp, vp, vp, vp]
    L.arp_amide_geometry.argtypes = [vp, i64, vp, vp, vp]
    L.arp_ring_residues.argtypes = [vp, i64, vp, vp, vp]
    L.arp_host_alloc.argtypes = [C.c_uint64, C.POINTER(C.c_void_p)]
    L.arp_host_free.argtypes = [vp]
    L.arp_stream_handle.argtypes = [vp]
    L.arp_use_stream.argtypes = [vp, C.c_uint64]
    L.arp_stream_handle.restype = C.c_uint64
    for s in SYMBOLS:
        f = getattr(L, s)
        if s not in ('arp_version', 'arp_last_error', 'arp_destroy', 'arp_stream_handle', 'arp_blob_size', 'arp_records_size',
                     'arp_cif_close', 'arp_cif_rows', 'arp_cif_tag', 'arp_cif_text'):
            f.restype = C.c_int
    _lib = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def batch_layout(boxes, radius):
    """Where arp_set_batch's grids put every structure at cell edge ``radius`` (arp_batch_layout: host arithmetic, no GPU;
    served by the host library where the HIP library has not been built).  ``boxes``: float64 [B, 6] = lo xyz, hi xyz.
    Returns ``dict(cell=int32 [B, 3] offsets, n=int32 [B, 3] cell counts, dims=(NX, NY, NZ), edge=float)``."""
    bx = np.ascontiguousarray(boxes, np.float64).reshape(-1, 6)
    B = bx.shape[0]
    places = np.zeros((max(B, 1), 6), np.int32)
    dims = np.zeros(3, np.int32)
    edge = C.c_double(0.0)
    rc = load_host().arp_batch_layout(B, _p(bx), float(radius), _p(places), _p(dims), C.byref(edge))
    if rc != ARP_OK:
        raise ValueError('arp_batch_layout: a box is not finite, has hi < lo or an infinite extent, or the radius is NaN')
    return dict(cell=places[:B, :3].copy(), n=places[:B, 3:].copy(), dims=tuple(int(v) for v in dims), edge=float(edge.value))


def pinned_empty(n, dtype):
    """NumPy array over page-locked memory from arp_host_alloc (freed when the array and its views are gone): the
    fetch calls fill such arrays at PCIe speed.  Falls back to ordinary memory when the allocation fails."""
    import weakref
    dt = np.dtype(dtype)
    nbytes = int(n) * dt.itemsize
    if nbytes == 0:
        return np.empty(int(n), dt)
    L = load()
    ptr = C.c_void_p()
    if L.arp_host_alloc(nbytes, C.byref(ptr)) != 0 or not ptr.value:
        return np.empty(int(n), dt)
    buf = (C.c_char * nbytes).from_address(ptr.value)
    weakref.finalize(buf, L.arp_host_free, C.c_void_p(ptr.value))
    return np.frombuffer(buf, dtype=dt, count=int(n))


class BlobHeader(C.Structure):
    """arp_blob_header of include/arpeggio_hip.h."""
    _fields_ = [('magic', C.c_uint64), ('bytes', C.c_uint64), ('n', C.c_int64), ('nres', C.c_int64), ('nbond', C.c_int64),
                ('nh', C.c_int64), ('nring', C.c_int64), ('namide', C.c_int64), ('n_rad', C.c_int64), ('off', C.c_uint64 * 21),
                ('lo', C.c_double * 3), ('hi', C.c_double * 3), ('ring_lo', C.c_double * 3), ('ring_hi', C.c_double * 3),
                ('amide_lo', C.c_double * 3), ('amide_hi', C.c_double * 3)]


_BLOB_DTYPES = (np.float32, np.float64, np.uint16, np.uint16, np.int32, np.uint8, np.int32, np.int32, np.int32, np.int32, np.int32,
                np.float64, np.int32, np.float64, np.float64, np.int32, np.float32, np.float32, np.int32, np.uint16, np.float64)


def pack_blob(pc, pinned=True):
    """The PackedComplex as ONE device-ready buffer (arp_blob_header + arrays, include/arpeggio_hip.h): a uint8 NumPy
    array over page-locked memory (``pinned``), ready for ``Context.set_blob``.  This is the packing step a producer of
    structures does once per structure; nothing is converted again on the way to the GPU."""
    L = load()
    n, nres, nring, namide = pc.n_atoms, pc.n_residues, pc.n_rings, pc.n_amides
    nbond, nh = int(pc.bond_idx.shape[0]), int(pc.h_xyz.shape[0])
    size = int(L.arp_blob_size(n, nres, nbond, nh, nring, namide))
    if size == 0:
        raise ValueError('pack_blob: counts out of range')
    buf = pinned_empty(size, np.uint8) if pinned else np.empty(size, np.uint8)
    if L.arp_blob_layout(_p(buf), size, n, nres, nbond, nh, nring, namide) != ARP_OK:
        raise ValueError('arp_blob_layout failed')
    c = lambda a, dt: np.ascontiguousarray(a, dt)
    arrays = [c(pc.xyz, np.float32), c(pc.vdw, np.float64), c(pc.cov, np.float64), c(pc.type_mask, np.uint16), c(pc.flags, np.uint16),
              c(pc.res_id, np.int32), c(pc.res_flags, np.uint8), c(pc.res_prev, np.int32), c(pc.res_next, np.int32),
              c(pc.bond_off, np.int32), c(pc.bond_idx, np.int32), c(pc.h_off, np.int32), c(pc.h_xyz, np.float64), c(pc.sb_nbr, np.int32),
              c(pc.ring_center, np.float64), c(pc.ring_normal, np.float64), c(pc.ring_res, np.int32), c(pc.amide_center, np.float32),
              c(pc.amide_normal, np.float32), c(pc.amide_res, np.int32)]
    if L.arp_blob_fill(_p(buf), size, *[_p(a) for a in arrays]) != ARP_OK:
        raise ValueError('arp_blob_fill failed')
    return buf


def unpack_blob(buf):
    """The arrays of a blob (as written by ``pack_blob`` or read back with ``Context.get_blob``) as a dict of NumPy views,
    radii decoded through the dictionary; for tests and tools."""
    hdr = BlobHeader.from_buffer_copy(buf[:C.sizeof(BlobHeader)].tobytes())
    n, nres, nring, namide, nbond, nh = int(hdr.n), int(hdr.nres), int(hdr.nring), int(hdr.namide), int(hdr.nbond), int(hdr.nh)
    counts = (4 * n, 2 * n, n, n, n, nres, nres, nres, n + 1, nbond, n + 1, 3 * nh, n, 3 * nring, 3 * nring, nring, 3 * namide,
              3 * namide, namide, n, 512)
    v = [np.frombuffer(buf, dtype=dt, count=cnt, offset=int(hdr.off[k])) for k, (dt, cnt) in enumerate(zip(_BLOB_DTYPES, counts))]
    names = ('xyz4', 'rad', 'type_mask', 'flags', 'res_id', 'res_flags', 'res_prev', 'res_next', 'bond_off', 'bond_idx', 'h_off',
             'h_xyz', 'sb_nbr', 'ring_center', 'ring_normal', 'ring_res', 'amide_center', 'amide_normal', 'amide_res', 'rad_idx',
             'rad_tab')
    d = dict(zip(names, v))
    d['xyz'] = d['xyz4'].reshape(-1, 4)[:, :3]
    d['rad'] = d['rad'].reshape(-1, 2)
    d['rad_tab'] = d['rad_tab'].reshape(256, 2)
    for k in ('h_xyz', 'ring_center', 'ring_normal', 'amide_center', 'amide_normal'):
        d[k] = d[k].reshape(-1, 3)
    d['header'] = hdr
    return d


# ---- record buffers of the device-side shard assembly (arp_rec_header / arp_rec_atom / ... of the header file) ----------
class RecHeader(C.Structure):
    _fields_ = [('magic', C.c_uint64), ('bytes', C.c_uint64), ('na', C.c_int64), ('nh', C.c_int64), ('nb', C.c_int64),
                ('nring', C.c_int64), ('namide', C.c_int64), ('n_rad', C.c_int64), ('off', C.c_uint64 * 5),
                ('lo', C.c_double * 3), ('hi', C.c_double * 3), ('ring_lo', C.c_double * 3), ('ring_hi', C.c_double * 3),
                ('amide_lo', C.c_double * 3), ('amide_hi', C.c_double * 3), ('rad_tab', C.c_double * 512)]


REC_ATOM = np.dtype([('xyz', '<f4', 3), ('gid', '<i4'), ('vdw', '<f8'), ('cov', '<f8'), ('sb_xyz', '<f4', 3), ('sb_has', '<i4'),
                     ('res_gid', '<i4'), ('res_prev', '<i4'), ('res_next', '<i4'), ('tmask', '<u2'), ('flags', '<u2'),
                     ('h_start', '<i4'), ('h_cnt', '<i4'), ('bond_start', '<i4'), ('bond_cnt', '<i4'),
                     ('res_flags', 'u1'), ('sel', 'u1'), ('pad', 'u1', 14)])
REC_RING = np.dtype([('c', '<f8', 3), ('n', '<f8', 3), ('gid', '<i4'), ('res', '<i4'), ('pad', '<i4', 2)])
REC_AMIDE = np.dtype([('c', '<f4', 3), ('n', '<f4', 3), ('gid', '<i4'), ('res', '<i4')])
assert REC_ATOM.itemsize == 96 and REC_RING.itemsize == 64 and REC_AMIDE.itemsize == 32


def _rec_views(buf, hdr):
    return (np.frombuffer(buf, REC_ATOM, int(hdr.na), int(hdr.off[0])), np.frombuffer(buf, np.float64, 3 * int(hdr.nh), int(hdr.off[1])).reshape(-1, 3),
            np.frombuffer(buf, np.int32, int(hdr.nb), int(hdr.off[2])), np.frombuffer(buf, REC_RING, int(hdr.nring), int(hdr.off[3])),
            np.frombuffer(buf, REC_AMIDE, int(hdr.namide), int(hdr.off[4])))


def pack_records_buffer(rec, pinned=True):
    """``sharding.pack_records`` output (dict of arrays, ascending ids) as ONE record buffer for ``Context.shard_set_home``."""
    L = load()
    na, nh, nb = int(rec['gid'].size), int(rec['h_xyz'].shape[0]), int(rec['bond_gid'].size)
    nr, nm = int(rec['ring_gid'].size), int(rec['amide_gid'].size)
    size = int(L.arp_records_size(na, nh, nb, nr, nm))
    if size == 0:
        raise ValueError('pack_records_buffer: counts out of range')
    buf = pinned_empty(size, np.uint8) if pinned else np.empty(size, np.uint8)
    buf[:] = 0
    if L.arp_records_layout(_p(buf), size, na, nh, nb, nr, nm) != ARP_OK:
        raise ValueError('arp_records_layout failed')
    hdr = RecHeader.from_buffer(buf)
    a, h, b, r, m = _rec_views(buf, hdr)
    a['xyz'], a['gid'], a['vdw'], a['cov'] = rec['xyz'], rec['gid'], rec['vdw'], rec['cov']
    a['sb_xyz'], a['sb_has'] = rec['sb_xyz'], rec['sb_has']
    a['res_gid'], a['res_prev'], a['res_next'], a['res_flags'] = rec['res_gid'], rec['res_prev'], rec['res_next'], rec['res_flags']
    a['tmask'], a['flags'], a['sel'] = rec['tmask'], rec['flags'], rec['sel']
    a['h_cnt'], a['bond_cnt'] = rec['h_cnt'], rec['bond_cnt']
    a['h_start'] = np.concatenate([[0], np.cumsum(rec['h_cnt'])])[:-1] if na else 0
    a['bond_start'] = np.concatenate([[0], np.cumsum(rec['bond_cnt'])])[:-1] if na else 0
    h[:], b[:] = rec['h_xyz'], rec['bond_gid']
    r['c'], r['n'], r['gid'], r['res'] = rec['ring_center'], rec['ring_normal'], rec['ring_gid'], rec['ring_res']
    m['c'], m['n'], m['gid'], m['res'] = rec['amide_center'], rec['amide_normal'], rec['amide_gid'], rec['amide_res']
    tab = np.zeros((256, 2))
    if na:
        keys = np.stack([rec['vdw'], rec['cov']], axis=1).astype(np.float64).view(np.uint64)
        uniq = np.unique(keys, axis=0)[:256]
        tab[:len(uniq)] = uniq.view(np.float64)
        hdr.n_rad = len(uniq)
    for k, val in enumerate(tab.reshape(-1)):
        hdr.rad_tab[k] = val
    for name, arr in (('', rec['xyz']), ('ring_', rec['ring_center']), ('amide_', rec['amide_center'])):
        lo = arr.min(axis=0).astype(np.float64) if len(arr) else np.zeros(3)
        hi = arr.max(axis=0).astype(np.float64) if len(arr) else np.zeros(3)
        for k in range(3):
            getattr(hdr, name + 'lo')[k] = lo[k]
            getattr(hdr, name + 'hi')[k] = hi[k]
    del hdr
    return buf


def pack_records_native(pc, atom_ids, ring_ids, amide_ids, sel=None, pinned=True):
    """The record buffer of the given atoms / rings / amides of ``pc`` (ascending packed indices = global ids), packed by the
    library (``arp_records_fill``): the same bytes as ``pack_records_buffer(sharding.pack_records(...))``, ~50x sooner."""
    L = load()
    a = np.ascontiguousarray(atom_ids, np.int64)
    r = np.ascontiguousarray(ring_ids, np.int64)
    m = np.ascontiguousarray(amide_ids, np.int64)
    h_off, b_off = np.ascontiguousarray(pc.h_off, np.int32), np.ascontiguousarray(pc.bond_off, np.int32)
    nh = int((h_off[a + 1] - h_off[a]).sum()) if a.size else 0
    nb = int((b_off[a + 1] - b_off[a]).sum()) if a.size else 0
    size = int(L.arp_records_size(a.size, nh, nb, r.size, m.size))
    if size == 0:
        raise ValueError('pack_records_native: counts out of range')
    buf = pinned_empty(size, np.uint8) if pinned else np.empty(size, np.uint8)
    if L.arp_records_layout(_p(buf), size, a.size, nh, nb, r.size, m.size) != ARP_OK:
        raise ValueError('arp_records_layout failed')
    c = lambda x, dt: np.ascontiguousarray(x, dt)
    arrays = [c(pc.xyz, np.float32), c(pc.vdw, np.float64), c(pc.cov, np.float64), c(pc.type_mask, np.uint16), c(pc.flags, np.uint16),
              c(pc.res_id, np.int32), c(pc.res_flags, np.uint8), c(pc.res_prev, np.int32), c(pc.res_next, np.int32), b_off,
              c(pc.bond_idx, np.int32), h_off, c(pc.h_xyz, np.float64), c(pc.sb_nbr, np.int32), c(pc.ring_center, np.float64),
              c(pc.ring_normal, np.float64), c(pc.ring_res, np.int32), c(pc.amide_center, np.float32), c(pc.amide_normal, np.float32),
              c(pc.amide_res, np.int32), (None if sel is None else c(sel, np.uint8)), a, r, m]
    if L.arp_records_fill(_p(buf), size, pc.n_atoms, pc.n_residues, pc.n_rings, pc.n_amides, *[_p(x) for x in arrays]) != ARP_OK:
        raise ValueError('arp_records_fill failed (ids must ascend and lie inside the structure)')
    return buf


def unpack_records_buffer(buf):
    """Inverse of ``pack_records_buffer`` (the dict ``sharding.pack_records`` makes); for tests."""
    hdr = RecHeader.from_buffer_copy(buf[:C.sizeof(RecHeader)].tobytes())
    a, h, b, r, m = _rec_views(buf, hdr)
    return {'gid': a['gid'].copy(), 'xyz': a['xyz'].copy(), 'vdw': a['vdw'].copy(), 'cov': a['cov'].copy(), 'tmask': a['tmask'].copy(),
            'flags': a['flags'].copy(), 'res_gid': a['res_gid'].copy(), 'res_flags': a['res_flags'].copy(), 'res_prev': a['res_prev'].copy(),
            'res_next': a['res_next'].copy(), 'sel': a['sel'].copy(), 'sb_xyz': a['sb_xyz'].copy(), 'sb_has': a['sb_has'].astype(np.uint8),
            'h_cnt': a['h_cnt'].copy(), 'h_xyz': h.copy(), 'bond_cnt': a['bond_cnt'].copy(), 'bond_gid': b.copy(),
            'h_start': a['h_start'].copy(), 'bond_start': a['bond_start'].copy(),
            'ring_gid': r['gid'].copy(), 'ring_center': r['c'].copy(), 'ring_normal': r['n'].copy(), 'ring_res': r['res'].copy(),
            'amide_gid': m['gid'].copy(), 'amide_center': m['c'].copy(), 'amide_normal': m['n'].copy(), 'amide_res': m['res'].copy(),
            'header': hdr}


class RowsBag(dict):
    """The atom-atom bag in ROWS layout (``Context.set_packed_layout(rows=True)``): ``row`` (N + 1 offsets) instead of ``i``;
    ``bag['i']`` is made from it on first use."""

    def __missing__(self, key):
        if key != 'i':
            raise KeyError(key)
        row = self['row']
        v = np.repeat(np.arange(len(row) - 1, dtype=np.int32), np.diff(row))
        self['i'] = v
        return v


class CifCategory:
    """One category of an mmCIF text (``arp_cif_open``): what gemmi's ``cif_block.get_mmcif_category(name)`` gives the
    reference — ``columns()[item]`` is a list with ``None`` for '?', ``False`` for '.', the unquoted string otherwise —
    plus bulk numeric access for the big ``_atom_site`` table."""

    def __init__(self, text, category):
        self._L = load_host()
        raw = text.encode('utf-8') if isinstance(text, str) else bytes(text)
        h, err = C.c_void_p(), C.create_string_buffer(256)
        rc = self._L.arp_cif_open(raw, len(raw), category.encode(), C.byref(h), err, 256)
        if rc != ARP_OK:
            raise ValueError(err.value.decode() or f'arp_cif_open failed ({rc})')
        self._h = h
        self.category = category
        self.rows, self.n_blocks = int(self._L.arp_cif_rows(h)), int(self._L.arp_cif_blocks(h))
        self.tags = [self._L.arp_cif_tag(h, k).decode() for k in range(int(self._L.arp_cif_cols(h)))]
        self._raw = raw

    def close(self):
        if getattr(self, '_h', None):
            self._L.arp_cif_close(self._h)
            self._h = None

    __del__ = close

    def __contains__(self, item):
        return item in self.tags

    def _cells(self, item):
        col = self.tags.index(item)
        b, ln, kd = np.empty(self.rows, np.uint64), np.empty(self.rows, np.uint32), np.empty(self.rows, np.uint8)
        if self._L.arp_cif_column(self._h, col, _p(b), _p(ln), _p(kd)) != ARP_OK:
            raise ValueError(f'arp_cif_column({item})')
        return b, ln, kd

    def column(self, item):
        """The column as gemmi delivers it: str / None ('?') / False ('.')."""
        b, ln, kd = self._cells(item)
        raw = self._raw
        return [raw[s:s + n].decode('utf-8') if k == 0 else (None if k == 1 else False)
                for s, n, k in zip(b.tolist(), ln.tolist(), kd.tolist())]

    def columns(self):
        return {t: self.column(t) for t in self.tags}

    def floats(self, item, missing=np.nan):
        out, bad = np.empty(self.rows, np.float64), C.c_int64(-1)
        if self._L.arp_cif_column_f64(self._h, self.tags.index(item), float(missing), _p(out), C.byref(bad)) != ARP_OK:
            raise ValueError(f'{self.category}{item}: row {bad.value} is not a number')
        return out

    def ints(self, item, missing=0):
        out, bad = np.empty(self.rows, np.int64), C.c_int64(-1)
        if self._L.arp_cif_column_i64(self._h, self.tags.index(item), int(missing), _p(out), C.byref(bad)) != ARP_OK:
            raise ValueError(f'{self.category}{item}: row {bad.value} is not an integer')
        return out


BAG_SORT_MAX = 8192       # ARP_BAG_SORT_MAX of include/arpeggio_hip.h
KERNEL_SLOTS = ('bin', 'scan', 'scatter', 'unused', 'search', 'sift', 'mark_search', 'planes')


# first-id column of every bag in its canonical order, and what its ids count (atoms / rings / amides)
_MODEL_SPLIT = {'atom_atom': ('i', {'i': 'n', 'j': 'n'}), 'atom_plane': ('ring', {'ring': 'nring', 'atom': 'n'}),
                'plane_plane': ('bgn', {'bgn': 'nring', 'end': 'nring'}), 'group_group': ('bgn', {'bgn': 'namide', 'end': 'namide'}),
                'group_plane': ('amide', {'amide': 'namide', 'ring': 'nring'})}


def split_models(bags, m):
    """The five bags of one pass over F resident models (arp_set_models) -> one dict of five bags per model, ids local to the
    model.  In each bag's canonical order the records of model f are ONE contiguous range — they follow those of model f - 1
    — so the cut is a binary search on the first-id column (in the ROWS layout: row[f n]), not a sort.  ``m``: the counts
    of one model (n, nring, namide) and F."""
    F = m['F']
    out = [dict() for _ in range(F)]
    for name, (key, shifts) in _MODEL_SPLIT.items():
        b = bags[name]
        if name == 'atom_atom' and isinstance(b, RowsBag):
            row = b['row']
            bounds = row[np.arange(F + 1) * m['n']].astype(np.int64)
            cols = {k: v for k, v in b.items() if k not in ('row', 'i')}
            for f in range(F):
                lo, hi = int(bounds[f]), int(bounds[f + 1])
                d = {k: v[lo:hi] for k, v in cols.items()}
                d['j'] = (d['j'] - f * m['n']).astype(np.int32)
                seg = row[f * m['n']:(f + 1) * m['n'] + 1]
                d['i'] = np.repeat(np.arange(m['n'], dtype=np.int32), np.diff(seg))
                out[f][name] = d
            continue
        bounds = np.searchsorted(b[key], np.arange(F + 1, dtype=np.int64) * m[shifts[key]], side='left')
        for f in range(F):
            lo, hi = int(bounds[f]), int(bounds[f + 1])
            d = {k: v[lo:hi] for k, v in b.items()}
            for col, what in shifts.items():
                d[col] = (d[col] - f * m[what]).astype(np.int32)
            out[f][name] = d
    return out


class Context:
    """One arp_ctx: one GPU, one HIP stream, device-resident structure."""

    def __init__(self, device: int = 0):
        self._L = load()
        h = C.c_void_p()
        rc = self._L.arp_create(int(device), C.byref(h))
        if rc != ARP_OK:
            msg = self._L.arp_last_error(None).decode()
            raise NativeLibraryError(f'arp_create(device={device}) failed ({rc}): {msg}')
        self._h = h
        self.device = device
        self.n = self.n_rings = self.n_amides = 0
        self._models = None          # counts of the resident models (set_models), None outside model mode
        # the five bag sizes of a pass land here (one context per host thread: no sharing); a ctypes array made once costs the
        # call nothing, a NumPy array + pointer per call cost ~2 us of a ~90 us pass
        self._counts = (C.c_int64 * 5)()
        self._counts_p = C.cast(self._counts, C.c_void_p)

    def close(self):
        if getattr(self, '_h', None):
            self._L.arp_destroy(self._h)
            self._h = None

    def set_grid_reuse(self, on=True):
        """Whole-structure passes keep their contact grid (default); ``False``: every pass builds it (measurements)."""
        self._check(self._L.arp_set_grid_reuse(self._h, int(bool(on))), 'arp_set_grid_reuse')

    def set_compact_lookback(self, on=True):
        """Every grid build finds its blocks' bases by look-back, also where the table made with the spatial order would serve
        (whole-structure passes); for tests that hold the two against each other."""
        self._check(self._L.arp_set_compact_lookback(self._h, int(bool(on))), 'arp_set_compact_lookback')

    def set_sort_after_pass(self, on=True):
        """``run_launch`` / ``run_wait`` enqueue the canonical sort of the atom-atom bag before they return (for callers that
        fetch the sorted bag next: ``fetch_packed``)."""
        self._check(self._L.arp_set_sort_after_pass(self._h, int(bool(on))), 'arp_set_sort_after_pass')

    def set_packed_layout(self, rows=False):
        """Layout of the atom-atom bag in ``fetch_packed`` (arp_set_packed_layout): records (a bgn id per record) or ROWS — ``row``:
        N + 1 offsets, the records of atom a are [row[a], row[a + 1]) — 4 bytes per record less over PCIe.  With rows the returned
        bag is a ``RowsBag``: ``bag['i']`` expands the offsets on first use (np.repeat), everything else is as before."""
        self._check(self._L.arp_set_packed_layout(self._h, 1 if rows else 0), 'arp_set_packed_layout')
        self._packed_rows = bool(rows)

    def device_synchronize(self):
        """Everything enqueued on this context's GPU has completed (the bracket of a timed region)."""
        self._check(self._L.arp_device_synchronize(self._h), 'arp_device_synchronize')

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc == ARP_OK:
            return
        msg = self._L.arp_last_error(self._h).decode()
        if rc == ARP_E_XBOND_NBR:
            # the reference dereferences None here (utils.py:173)
            raise AttributeError("'NoneType' object has no attribute 'GetId'")
        if rc == ARP_E_ARG:
            raise ValueError(f'{what}: {msg}')
        err = NativeLibraryError(f'{what} failed ({rc}): {msg}')
        err.code = rc
        raise err

    # ---- inputs ----
    def set_complex(self, pc):
        """Upload a PackedComplex (everything initialize() leaves behind)."""
        L, h = self._L, self._h
        self._keep = pc
        self._check(L.arp_set_atoms(h, pc.n_atoms, _p(pc.xyz), _p(pc.vdw), _p(pc.cov), _p(pc.type_mask), _p(pc.flags),
                                    _p(pc.res_id)), 'arp_set_atoms')
        self._check(L.arp_set_residues(h, pc.n_residues, _p(pc.res_flags), _p(pc.res_prev), _p(pc.res_next)), 'arp_set_residues')
        self._check(L.arp_set_bonds(h, _p(pc.bond_off), _p(pc.bond_idx)), 'arp_set_bonds')
        self._check(L.arp_set_hydrogens(h, _p(pc.h_off), _p(pc.h_xyz)), 'arp_set_hydrogens')
        self._check(L.arp_set_single_bond_neighbours(h, _p(pc.sb_nbr)), 'arp_set_single_bond_neighbours')
        self._check(L.arp_set_rings(h, pc.n_rings, _p(pc.ring_center), _p(pc.ring_normal), _p(pc.ring_res)), 'arp_set_rings')
        self._check(L.arp_set_amides(h, pc.n_amides, _p(pc.amide_center), _p(pc.amide_normal), _p(pc.amide_res)), 'arp_set_amides')
        self.n, self.n_rings, self.n_amides = pc.n_atoms, pc.n_rings, pc.n_amides
        self._models = None
        self._sel = None             # (a new structure starts with everything selected)

    def set_batch(self, pcs, selections=None):
        """Several structures in one pass (arpeggio_amd.batch): uploads the concatenation of ``pcs`` and tells the library
        where each structure begins.  ``selections``: per-structure uint8 masks (None = whole structure).  Returns the
        offsets that ``run_batch`` / ``batch.split_*`` use."""
        from . import batch as _batch
        big, off = _batch.concat_complexes(pcs)
        self.set_complex(big)
        self.declare_batch(off)
        if selections is not None:
            sel = np.concatenate([np.ones(pc.n_atoms, np.uint8) if s_ is None else np.asarray(s_, np.uint8) for pc, s_ in zip(pcs, selections)])
            self.set_selection(sel)
        return off

    def declare_batch(self, off):
        """Tell the library how the resident (concatenated) structure splits into structures: ``off`` as returned by
        ``batch.concat_complexes`` (after ``set_complex`` / ``set_blob`` of the concatenation)."""
        a, r, m, bx = (np.ascontiguousarray(off[k]) for k in ('atom', 'ring', 'amide', 'boxes'))
        self._check(self._L.arp_set_batch(self._h, len(a) - 1, _p(a), _p(r), _p(m), _p(bx)), 'arp_set_batch')
        self._batch = off
        self._models = None

    def run_batch(self, cutoff=5.0, vdw_comp=0.1, include_sequence_adjacent=False, expand_radius=6.0, fetch=True):
        """run_arpeggio on every structure of the resident batch in ONE pass.  Returns a list of per-structure dicts
        {atom_atom, atom_plane, plane_plane, group_group, group_plane} with structure-local ids, canonically sorted."""
        from . import batch as _batch
        counts = self.run_launch(cutoff, vdw_comp, include_sequence_adjacent, expand_radius)
        if not fetch:
            return counts
        off = self._batch
        per = [dict() for _ in range(len(off['atom']) - 1)]
        for s_, d in enumerate(_batch.split_atom_contacts(self.atom_contacts_fetch(counts['atom_atom'], sort=True), off)):
            per[s_]['atom_atom'] = d
        for name in ('atom_plane', 'plane_plane', 'group_group', 'group_plane'):
            for s_, d in enumerate(_batch.split_bag(name, self.fetch_bag(name, sort=True), off)):
                per[s_][name] = d
        return per

    # ---- one topology, several models (arp_set_topology / arp_set_models) ----
    def set_topology(self, pc):
        """Keep ``pc``'s topology on the device (its coordinates are model 1's; ring / amide centres are not read):
        ``pc.ring_atoms`` in ring-path order and ``pc.amide_atoms`` (N, C, O, C-alpha) are what every model's planes are made
        from.  The resident structure is not touched."""
        blob = pack_blob(pc, pinned=False)
        nr = pc.n_rings
        if nr and len(pc.ring_atoms) != nr:
            raise ValueError('set_topology: the pack needs the atoms of every ring (ring_atoms)')
        off = np.zeros(nr + 1, np.int32)
        off[1:] = np.cumsum([len(a) for a in pc.ring_atoms]) if nr else []
        idx = np.ascontiguousarray(np.concatenate([np.asarray(a, np.int32) for a in pc.ring_atoms]) if nr else np.zeros(1, np.int32))
        am = np.ascontiguousarray(pc.amide_atoms, np.int32).reshape(-1, 4)
        self._check(self._L.arp_set_topology(self._h, _p(blob), int(blob.nbytes), _p(off), _p(idx), _p(am)), 'arp_set_topology')
        self._topology = dict(n=pc.n_atoms, nres=pc.n_residues, nring=nr, namide=pc.n_amides, nh=int(pc.h_xyz.shape[0]))

    def set_models(self, xyz, h_xyz):
        """F models of the kept topology become the resident structure, one batch partition per model:
        ``xyz`` float32 [F, n, 3], ``h_xyz`` float64 [F, nh, 3] (hydrogens in the topology's h_off order)."""
        t = getattr(self, '_topology', None)
        if t is None:
            raise ValueError('set_models: no topology (set_topology first)')
        x = np.ascontiguousarray(xyz, np.float32)
        hx = np.ascontiguousarray(h_xyz, np.float64)
        if x.ndim != 3 or x.shape[1:] != (t['n'], 3):
            raise ValueError(f'set_models: xyz must be [F, {t["n"]}, 3]')
        F = x.shape[0]
        if hx.shape != (F, t['nh'], 3):
            raise ValueError(f'set_models: h_xyz must be [{F}, {t["nh"]}, 3]')
        self._models = None
        self._sel = None
        self.n = self.n_rings = self.n_amides = 0      # (a failed call leaves nothing resident)
        self._check(self._L.arp_set_models(self._h, F, _p(x), _p(hx)), 'arp_set_models')
        self.n, self.n_rings, self.n_amides = F * t['n'], F * t['nring'], F * t['namide']
        self._models = dict(t, F=F)

    def models_planes(self):
        """Per model: ring_center / ring_normal f64 [F, R, 3], ring_res i32 [F, R] (residues of the model, -1 = none),
        amide_center / amide_normal f32 [F, A, 3] — what set_models computed on the device."""
        m = self._models
        if m is None:
            raise ValueError('models_planes: no models resident (set_models)')
        F, R, A = m['F'], m['nring'], m['namide']
        rc, rn, rr = np.zeros((F, R, 3)), np.zeros((F, R, 3)), np.zeros((F, R), np.int32)
        ac, an = np.zeros((F, A, 3), np.float32), np.zeros((F, A, 3), np.float32)
        self._check(self._L.arp_models_planes(self._h, _p(rc), _p(rn), _p(rr), _p(ac), _p(an)), 'arp_models_planes')
        return dict(ring_center=rc, ring_normal=rn, ring_res=rr, amide_center=ac, amide_normal=an)

    def run_models(self, cutoff=5.0, vdw_comp=0.1, include_sequence_adjacent=False, expand_radius=6.0, contact_filter=None):
        """run_arpeggio on every resident model in ONE pass; one ``fetch_packed``, cut into the models by contiguous ranges
        (``split_models``).  Returns a list of F dicts {atom_atom, atom_plane, plane_plane, group_group, group_plane} with
        model-local ids.  ``contact_filter``: (sift_any, ctype_mask) — the fetch is ``fetch_packed_filtered``, every model's
        atom-atom bag its kept records."""
        if self._models is None:
            raise ValueError('run_models: no models resident (set_models)')
        self.run_launch(cutoff, vdw_comp, include_sequence_adjacent, expand_radius)
        bags, _ = self.fetch_packed() if contact_filter is None else self.fetch_packed_filtered(*contact_filter)
        return split_models(bags, self._models)

    def _table(self, launch, fetch, spec, *args):
        """One device-reduced table: launch with its arguments ``args`` (the row count), then one fetch of every column of
        ``spec``."""
        n = C.c_int64(0)
        self._check(getattr(self._L, launch)(self._h, *args, C.byref(n)), launch)
        U = int(n.value)
        t = tables.alloc(spec, U)
        self._check(getattr(self._L, fetch)(self._h, U, *(_p(t[k]) for k, _ in spec.columns), C.byref(n)), fetch)
        return t

    def models_persistence(self):
        """Contact persistence over the resident models of the last pass, reduced on the device (arp_models_persistence_*):
        one row per distinct topology pair (a, b) in ascending (a, b).  Returns a dict of the ten columns ``PERSIST_COLUMNS``
        (``bit_count`` as [U, 15]; see ``arpeggio_amd.persistence``).  Only the table is copied to the host; the bags of the
        pass stay fetchable as before."""
        return self._table('arp_models_persistence_launch', 'arp_models_persistence_fetch', tables.PERSIST)

    def residue_pairs(self):
        """The residue-residue contact table of the last complete pass, reduced on the device (arp_residue_pairs_*): one row
        per unordered residue pair with a record in any of the five bags, rows in ascending (res_a, res_b).  Returns a dict
        of the seven columns ``RESPAIR_COLUMNS`` (``bit_count`` as [U, 15], ``plane_count`` as [U, 4]; see
        ``arpeggio_amd.residue_pairs``).  Only the table is copied to the host; the bags of the pass stay fetchable as
        before.  With a batch or models resident the ids are those of the concatenation (``residue_pairs.split``)."""
        return self._table('arp_residue_pairs_launch', 'arp_residue_pairs_fetch', tables.RESPAIR)

    def models_residue_persistence(self):
        """Residue contact persistence over the resident models of the last complete pass, reduced on the device
        (arp_models_residue_persistence_*): one row per pair of topology residues with a record in any bag of any model,
        rows in ascending (res_a, res_b).  Returns a dict of the twelve columns ``RESPERSIST_COLUMNS`` (``class_models`` as
        [U, 5], ``bit_models`` as [U, 15]; see ``arpeggio_amd.residue_persistence``).  Only the table is copied to the host;
        the bags of the pass and the two other tables stay fetchable as before."""
        return self._table('arp_models_residue_persistence_launch', 'arp_models_residue_persistence_fetch', tables.RESPERSIST)

    def water_bridges(self, sift_any, flags=0):
        """The water-mediated contacts of the last pass, joined on the device (arp_water_bridges_*): one row per water and
        unordered pair of its partners, rows in ascending (water, a, b).  A leg is a record with exactly one water atom and
        ``(sift & sift_any) != 0``; ``flags``: ``water_bridges.SAME_RESIDUE`` keeps the pairs of one residue.  Returns a dict of
        the nine columns ``water_bridges.COLUMNS`` (see ``arpeggio_amd.water_bridges``).  Only the table is copied to the host;
        the bags of the pass, the filtered bag and the three tables stay fetchable as before.  With a batch or models resident
        the ids are those of the concatenation (``water_bridges.split_structures`` / ``split_models``)."""
        return self._table('arp_water_bridges_launch', 'arp_water_bridges_fetch', tables.BRIDGES, int(sift_any), int(flags))

    def models_water_bridge_persistence(self, sift_any, flags=0):
        """Water-bridge persistence over the resident models of the last pass, reduced on the device
        (arp_models_water_bridge_persistence_*): the bridge table of ``water_bridges(sift_any, flags & SAME_RESIDUE)`` folded
        per pair of topology atoms — or, with ``WBP_BY_RESIDUE`` in ``flags``, of topology residues —, rows ascending by the
        pair.  Returns a dict of the fourteen columns ``tables.BRIDGEPERSIST_ATOM`` / ``BRIDGEPERSIST_RESIDUE``
        (``bit_models_a`` / ``bit_models_b`` as [U, 15]; see ``arpeggio_amd.bridge_persistence``).  Only the table is copied to
        the host; the bridge table stays resident and fetchable, and every other result stays what it was."""
        spec = tables.BRIDGEPERSIST_RESIDUE if int(flags) & WBP_BY_RESIDUE else tables.BRIDGEPERSIST_ATOM
        return self._table('arp_models_water_bridge_persistence_launch', 'arp_models_water_bridge_persistence_fetch', spec,
                           int(sift_any), int(flags))

    def models_similarity(self, planes, ctype_mask=CTYPE_ALL, by_residue=False):
        """The model-by-model matrix of shared interaction features of the last pass, made on the device
        (arp_models_similarity_*): ``inter`` uint32 [F, F], ``inter[f, g]`` = features (row, plane) present in model f and in
        model g — rows the topology atom pairs of ``models_persistence`` or, with ``by_residue``, the topology residue pairs of
        ``models_residue_persistence`` (a complete pass); ``planes`` as ``similarity.planes`` builds it; an atom-atom record
        takes part when bit ``ctype`` of ``ctype_mask`` is set (see ``arpeggio_amd.similarity``).  Only the matrix is copied to
        the host; the bags of the pass and every table stay fetchable as before.  The row count and what the launch did are in
        ``stats()`` (``sim_rows``, ``sim_words``, ``sim_slices``, ``sim_launches``)."""
        F, U = C.c_int64(0), C.c_int64(0)
        flags = SIM_BY_RESIDUE if by_residue else 0
        self._check(self._L.arp_models_similarity_launch(self._h, int(planes), int(ctype_mask), flags, C.byref(F), C.byref(U)),
                    'arp_models_similarity_launch')
        n = int(F.value)
        inter = np.empty((n, n), np.uint32)
        self._check(self._L.arp_models_similarity_fetch(self._h, n, _p(inter), C.byref(F)), 'arp_models_similarity_fetch')
        return inter

    def models_coupling(self, planes, ctype_mask=CTYPE_ALL, by_residue=False, min_count=1, max_count=None, phi2_q=512, max_pairs=1 << 20):
        """Contact coupling over the resident models of the last pass, correlated on the device (arp_models_coupling_*): which
        contacts form and break together.  A row — a topology atom pair of ``models_persistence`` or, ``by_residue``, a topology
        residue pair of ``models_residue_persistence`` (a complete pass) — is present in a model when a participating record of
        it has a plane of ``planes`` (``similarity.planes``; bit ``ctype`` of ``ctype_mask`` decides participation).  The rows
        present in ``min_count`` ... ``max_count`` models (``None``: F - 1) are the features; a pair of features is kept when
        phi^2 >= ``phi2_q`` / 1024 (``coupling.phi2_q``).  Returns ``(features, pairs)``, dicts of the columns
        ``tables.COUPLING_FEATURES`` (a, b, count) and ``tables.COUPLING_PAIRS`` (u, v, n11), in ascending (a, b) and (u, v); see
        ``arpeggio_amd.coupling``.  More kept pairs than ``max_pairs``: ``NativeLibraryError`` with ``code`` ARP_E_CAPACITY and
        the exact number in ``n_pairs``.  Only the two tables are copied to the host; the bags of the pass and every other
        result stay fetchable as before.  What the launch did is in ``stats()`` (``couple_rows``, ``couple_features``,
        ``couple_tile_pairs``, ``couple_launches``)."""
        if self._models is None:
            raise ValueError('models_coupling: no models resident (set_models)')
        K, P = C.c_int64(0), C.c_int64(0)
        top = self._models['F'] - 1 if max_count is None else int(max_count)
        rc = self._L.arp_models_coupling_launch(self._h, int(planes), int(ctype_mask), COUPLE_BY_RESIDUE if by_residue else 0, int(min_count),
                                                max(top, 0), int(phi2_q), int(max_pairs), C.byref(K), C.byref(P))
        try:
            self._check(rc, 'arp_models_coupling_launch')
        except NativeLibraryError as e:
            e.n_features, e.n_pairs = int(K.value), int(P.value)
            raise
        f, t = tables.alloc(tables.COUPLING_FEATURES, int(K.value)), tables.alloc(tables.COUPLING_PAIRS, int(P.value))
        self._check(self._L.arp_models_coupling_fetch(self._h, int(K.value), int(P.value), *(_p(f[k]) for k, _ in tables.COUPLING_FEATURES.columns),
                                                      *(_p(t[k]) for k, _ in tables.COUPLING_PAIRS.columns), C.byref(K), C.byref(P)),
                    'arp_models_coupling_fetch')
        return f, t

    def models_lifetimes(self, gap=0, sift_any=0x7FFF, ctype_mask=CTYPE_ALL):
        """Contact lifetimes over the resident models of the last pass, reduced on the device (arp_models_lifetimes_*): per
        topology pair (a, b) with a participating record — ``(sift & sift_any) != 0`` and bit ``ctype`` of ``ctype_mask`` set —
        the intervals of its presence along the model axis, ``gap`` models of absence tolerated inside one; rows in ascending
        (a, b).  Returns a dict of the eleven columns ``tables.LIFETIMES`` (see ``arpeggio_amd.lifetimes``).  Only the table is
        copied to the host; the bags of the pass and every other result stay fetchable as before.  A repeated call with the
        same arguments on the same results fetches the resident table (``stats()['lifetimes_launches']`` counts the launches
        that made one)."""
        return self._table('arp_models_lifetimes_launch', 'arp_models_lifetimes_fetch', tables.LIFETIMES, int(gap), int(sift_any),
                           int(ctype_mask))

    def networks(self, sift_any=0x7FFF, ctype_mask=CTYPE_ALL, by_residue=False):
        """Interaction networks of the last pass: the connected components of the contact graph, labelled on the device
        (arp_networks_*).  Nodes are the resident atoms or, ``by_residue``, the resident residues; an atom-atom record is an edge
        when ``(sift & sift_any) != 0`` and bit ``ctype`` of ``ctype_mask`` is set.  Returns ``(label, table)``: ``label`` int32
        [N], the smallest node id of each node's component or -1 for a node without a participating record, and a dict of
        the five columns ``tables.NETWORKS``, one row per component in ascending ``root`` (see ``arpeggio_amd.networks``).
        Only the labels and the table are copied to the host; the bags of the pass and every other result stay fetchable as
        before.  With a batch or models resident the ids are those of the concatenation (``networks.split_structures`` /
        ``split_models``).  A repeated call with the same arguments on the same results fetches the resident result
        (``stats()['networks_launches']`` counts the launches that made one)."""
        table = self._table('arp_networks_launch', 'arp_networks_fetch', tables.NETWORKS, int(sift_any), int(ctype_mask),
                            NET_BY_RESIDUE if by_residue else 0)
        info = np.zeros(3, np.int64)
        self._check(self._L.arp_networks_info(self._h, _p(info)), 'arp_networks_info')
        N = C.c_int64(0)
        label = np.empty(int(info[1]), np.int32)
        self._check(self._L.arp_networks_labels_fetch(self._h, len(label), _p(label), C.byref(N)), 'arp_networks_labels_fetch')
        return label, table

    def _pose_records_fetch(self, entry, second, P, k):
        """The fetch of a launch over ``P`` poses with ``k`` records through C entry ``entry`` (arp_poses_contacts_fetch or
        arp_library_contacts_fetch): a dict of the five columns — ``second`` names the second id column —, ``pose_off`` and
        ``summary``; with ``second`` None only the summary, as an array."""
        summary = np.empty((P, POSES_SUMMARY), np.uint32)
        t = {}
        if second is not None:
            t = {'i': np.empty(k, np.int32), second: np.empty(k, np.int32), 'dist': np.empty(k, np.float32), 'sift': np.empty(k, np.uint16),
                 'ctype': np.empty(k, np.uint8), 'pose_off': np.empty(P + 1, np.uint64), 'summary': summary}
        n = C.c_int64(0)
        self._check(getattr(self._L, entry)(self._h, k, *(_p(t[c]) if t else None for c in ('pose_off', 'i', second, 'dist', 'sift', 'ctype')),
                                            _p(summary), C.byref(n)), entry)
        return t if t else summary

    def _poses_launch(self, xyz, h_xyz, cutoff, vdw_comp, include_sequence_adjacent):
        """Shapes checked against the uploaded selection, then arp_poses_contacts_launch; returns (P, records, movable ids)."""
        sel = getattr(self, '_sel', None)
        if sel is None or len(sel) != self.n:
            raise ValueError('poses_contacts: no uploaded selection (set_selection names the movable set)')
        atoms = np.nonzero(sel)[0].astype(np.int32)
        S = len(atoms)
        x = np.ascontiguousarray(xyz, np.float32)
        if x.ndim != 3 or x.shape[1:] != (S, 3) or x.shape[0] < 1:
            raise ValueError(f'poses_contacts: xyz must be [P >= 1, {S}, 3] (the selected atoms in ascending order)')
        P = x.shape[0]
        hx = np.zeros((P, 0, 3)) if h_xyz is None else np.ascontiguousarray(h_xyz, np.float64)
        # (the library reads P * SH rows: the shape is checked here, where the hydrogen offsets of the resident structure are known)
        keep = getattr(self, '_keep', None)
        h_off = getattr(keep, 'h_off', None)
        if h_off is None and isinstance(keep, np.ndarray):
            h_off = unpack_blob(keep)['h_off']
        if h_off is None or len(h_off) != self.n + 1:
            raise ValueError('poses_contacts: the hydrogen offsets of the resident structure are not known to this context')
        SH = int(np.diff(np.asarray(h_off, np.int64))[atoms].sum()) if S else 0
        if hx.shape != (P, SH, 3):
            raise ValueError(f'poses_contacts: h_xyz must be [{P}, {SH}, 3] (the hydrogen rows of the selected atoms, h_off order)')
        n = C.c_int64(0)
        rc = self._L.arp_poses_contacts_launch(self._h, P, _p(x), _p(hx) if SH else None, float(cutoff), float(vdw_comp),
                                               int(bool(include_sequence_adjacent)), C.byref(n))
        try:
            self._check(rc, 'arp_poses_contacts_launch')
        except NativeLibraryError as e:
            e.n_records = int(n.value)
            raise
        return P, int(n.value), atoms

    def poses_contacts(self, xyz, h_xyz, cutoff=5.0, vdw_comp=0.1, include_sequence_adjacent=False):
        """Every pose's ligand - receptor contacts in one launch (arp_poses_contacts_*; ``arpeggio_amd.poses``).  The uploaded
        selection is the movable set; ``xyz`` float32 [P, S, 3] its atoms' coordinates per pose (ascending packed order),
        ``h_xyz`` float64 [P, SH, 3] the hydrogen rows of those atoms (``poses.movable`` gives both index lists).  Returns a dict:
        ``i, j, dist, sift, ctype`` — per pose exactly the atom-atom records with one selected and one unselected atom of a pass
        over the structure with the pose scattered in, in ascending (pose, i, j) —, ``pose_off`` uint64 [P + 1], ``summary``
        uint32 [P, 16] (records per SIFt bit, slot 15 the total) and ``movable`` (the selected atom ids).  At most
        ``POSES_MAX_POSES`` poses a call (``poses.concat`` joins chunks); ``cutoff`` <= 6.0.  The bags of the last pass and
        every table made from them stay as they are."""
        P, k, atoms = self._poses_launch(xyz, h_xyz, cutoff, vdw_comp, include_sequence_adjacent)
        t = self._pose_records_fetch('arp_poses_contacts_fetch', 'j', P, k)
        t['movable'] = atoms
        return t

    def poses_summary(self, xyz, h_xyz, cutoff=5.0, vdw_comp=0.1, include_sequence_adjacent=False):
        """``poses_contacts`` with only the per-pose summary copied to the host: uint32 [P, 16], records per SIFt bit and, in
        slot 15, all records of the pose — for ranking many poses without copying a record."""
        P, _, _ = self._poses_launch(xyz, h_xyz, cutoff, vdw_comp, include_sequence_adjacent)
        return self._pose_records_fetch('arp_poses_contacts_fetch', None, P, 0)

    def poses_info(self):
        """(P, S, SH, records) of the resident poses result, zeros while there is none (arp_poses_contacts_info)."""
        info = np.zeros(4, np.int64)
        self._check(self._L.arp_poses_contacts_info(self._h, _p(info)), 'arp_poses_contacts_info')
        return dict(poses=int(info[0]), atoms=int(info[1]), hydrogens=int(info[2]), records=int(info[3]))

    def set_plane_atoms(self, pc):
        """The atoms of the resident rings and amides (arp_set_plane_atoms): ``pc.ring_atoms`` in ring-path order and
        ``pc.amide_atoms`` (N, C, O, C-alpha) of the structure that is resident.  What ``poses_planes`` rebuilds a pose's ring
        and amide geometry from; dropped with the structure, its rings or its amides."""
        nr, na = pc.n_rings, pc.n_amides
        if nr != self.n_rings or na != self.n_amides or pc.n_atoms != self.n:
            raise ValueError('set_plane_atoms: counts differ from the resident structure')
        if nr and len(pc.ring_atoms) != nr:
            raise ValueError('set_plane_atoms: the pack needs the atoms of every ring (ring_atoms)')
        off = np.zeros(nr + 1, np.int32)
        off[1:] = np.cumsum([len(a) for a in pc.ring_atoms]) if nr else []
        idx = np.ascontiguousarray(np.concatenate([np.asarray(a, np.int32) for a in pc.ring_atoms]) if nr else np.zeros(1, np.int32))
        am = np.ascontiguousarray(pc.amide_atoms, np.int32).reshape(-1, 4)
        if len(am) != na:
            raise ValueError('set_plane_atoms: counts differ from the resident structure (amide_atoms)')
        self._check(self._L.arp_set_plane_atoms(self._h, _p(off), _p(idx), _p(am) if na else None), 'arp_set_plane_atoms')

    def _poses_planes_launch(self, xyz):
        sel = getattr(self, '_sel', None)
        if sel is None or len(sel) != self.n:
            raise ValueError('poses_planes: no uploaded selection (set_selection names the movable set)')
        atoms = np.nonzero(sel)[0].astype(np.int32)
        S = len(atoms)
        x = np.ascontiguousarray(xyz, np.float32)
        if x.ndim != 3 or x.shape[1:] != (S, 3) or x.shape[0] < 1:
            raise ValueError(f'poses_planes: xyz must be [P >= 1, {S}, 3] (the selected atoms in ascending order)')
        counts = np.zeros(4, np.int64)
        self._check(self._L.arp_poses_planes_launch(self._h, x.shape[0], _p(x), _p(counts)), 'arp_poses_planes_launch')
        return x.shape[0], counts, atoms

    @staticmethod
    def _plane_table_buffers(name, k, n_off):
        """A ring / amide table of ``k`` records with ``pose_off`` [n_off], and its columns as the pointers of a plane fetch (two
        ids, four values, three bytes: ``tables.BAGS``; the columns the table does not have are null)."""
        b = tables.BAGS[name]
        tab = {c: np.empty(k, dt) for c, dt, _ in tables.bag_columns(name)}
        args = [_p(tab[c]) for c, _ in b.ids] + [_p(tab[c]) for c in b.vals] + [None] * (4 - len(b.vals)) + [_p(tab[c]) for c in b.bytes] + [None] * (3 - len(b.bytes))
        tab['pose_off'] = np.empty(n_off, np.uint64)
        return tab, args

    def poses_planes(self, xyz):
        """Every pose's ring and amide contacts in one launch (arp_poses_planes_*; ``arpeggio_amd.poses``).  The uploaded selection
        is the movable set, ``set_plane_atoms`` has named the ring and amide atoms; ``xyz`` float32 [P, S, 3].  Returns a dict with
        one table per bag — ``atom_plane``, ``plane_plane``, ``group_group``, ``group_plane``: the columns of ``fetch_bag`` plus
        ``pose_off`` uint64 [P + 1], per pose exactly the records of the posed structure's bag that involve an affected entity
        (``poses.affected``), in the bag's canonical order —, ``summary`` uint32 [P, 16] and ``movable``."""
        from . import poses as _poses
        P, counts, atoms = self._poses_planes_launch(xyz)
        out = {}
        n = C.c_int64(0)
        summary = np.empty((P, POSES_PLANES_SUMMARY), np.uint32)
        for t, name in enumerate(_poses.PLANE_TABLES):
            k = int(counts[t])
            tab, args = self._plane_table_buffers(name, k, P + 1)
            self._check(self._L.arp_poses_planes_fetch(self._h, t, k, _p(tab['pose_off']), *args, _p(summary) if t == 0 else None, C.byref(n)),
                        'arp_poses_planes_fetch')
            out[name] = tab
        out['summary'] = summary
        out['movable'] = atoms
        return out

    def poses_planes_summary(self, xyz):
        """``poses_planes`` with only the per-pose summary copied to the host: uint32 [P, 16] (slots: ``poses.PLANE_SUMMARY_SLOTS``)."""
        P, _, _ = self._poses_planes_launch(xyz)
        s = np.empty((P, POSES_PLANES_SUMMARY), np.uint32)
        n = C.c_int64(0)
        self._check(self._L.arp_poses_planes_fetch(self._h, 0, 0, *([None] * 10), _p(s), C.byref(n)), 'arp_poses_planes_fetch')
        return s

    def poses_planes_info(self):
        """arp_poses_planes_info: poses, atoms and records per table of the resident result (zeros while there is none), the sizes of
        the movable set's lists, whether plane atoms are resident, and the kernel launches so far."""
        from . import poses as _poses
        info = np.zeros(12, np.int64)
        self._check(self._L.arp_poses_planes_info(self._h, _p(info)), 'arp_poses_planes_info')
        d = dict(poses=int(info[0]), atoms=int(info[1]))
        d.update({name: int(info[2 + t]) for t, name in enumerate(_poses.PLANE_TABLES)})
        d.update(moved_rings=int(info[6]), home_rings=int(info[7]), moved_amides=int(info[8]), plane_atoms=bool(info[9]), launches=int(info[10]))
        return d

    def poses_fingerprints(self, planes, ctype_mask=CTYPE_ALL, by_residue=True, n_refs=0, all_pairs=False, bits=False):
        """The resident poses result (``poses_contacts`` / ``poses_summary``) reduced on the device to interaction fingerprints
        and their scores (arp_poses_fingerprints_*; ``arpeggio_amd.pose_fingerprints``).  The first ``n_refs`` poses of that
        launch are the references (at most ``POSEFP_MAX_REFS``).  A feature is (node, plane): the receptor residue
        (``by_residue=False``: receptor atom) of a record whose ``ctype`` bit is in ``ctype_mask``, and one of the SIFt bits of
        ``planes`` (``pose_fingerprints.planes``) the record has.  Returns a dict: ``ids`` int32 [U], the nodes that occur,
        ascending; ``count`` uint32 [P], features per pose; ``cross`` uint32 [P, n_refs], features a pose shares with a
        reference; ``occupancy`` uint32 [U, NP], poses behind the references that have the feature; ``planes``, ``n_refs``,
        ``level``; with ``bits=True`` the bit matrix ``bits`` uint64 [P, NP, ceil(U / 64)]; with ``all_pairs=True`` (at most
        ``SIM_MAX_MODELS`` poses) ``inter`` uint32 [P, P].  No record is copied.  A repeated call with the same arguments on
        the same poses result launches nothing (``poses_fingerprints_info()['launches']``).

        A ``planes`` mask with a bit from ``POSEFP_PLANES`` on (``pose_fingerprints.planes(classes=...)``) adds the ring and amide
        classes as planes (arp_poses_fingerprints_planes_launch): the resident ``poses_planes`` result of the SAME poses is
        reduced into the same matrix, residue level only; ``planes`` in the result is the unified mask."""
        flags = (POSEFP_BY_RESIDUE if by_residue else 0) | (POSEFP_ALL_PAIRS if all_pairs else 0)
        info = np.zeros(8, np.int64)
        entry = 'arp_poses_fingerprints_planes_launch' if int(planes) >> POSEFP_PLANES else 'arp_poses_fingerprints_launch'
        self._check(getattr(self._L, entry)(self._h, int(planes), int(ctype_mask), flags, int(n_refs), _p(info)), entry)
        P, Q, U, NP, W = (int(v) for v in info[:5])
        NP = bin(int(planes)).count('1')      # (what info[3] holds)
        out = dict(ids=np.empty(U, np.int32), count=np.empty(P, np.uint32), cross=np.empty((P, Q), np.uint32),
                   occupancy=np.empty((U, NP), np.uint32))
        if bits:
            out['bits'] = np.empty((P, NP, (U + 63) // 64), np.uint64)
        if all_pairs:
            out['inter'] = np.empty((P, P), np.uint32)
        n = C.c_int64(0)
        self._check(self._L.arp_poses_fingerprints_fetch(self._h, U, _p(out['ids']), _p(out['count']), _p(out['cross']), _p(out['occupancy']),
                                                         _p(out.get('bits')), _p(out.get('inter')), C.byref(n)), 'arp_poses_fingerprints_fetch')
        out.update(planes=int(planes), n_refs=Q, level='residue' if by_residue else 'atom')
        return out

    def poses_fingerprints_info(self):
        """arp_poses_fingerprints_info: poses, references, columns, planes, words per pose and word slices of the resident
        fingerprint result (zeros while there is none), the launches that did work so far, and the flags."""
        info = np.zeros(8, np.int64)
        self._check(self._L.arp_poses_fingerprints_info(self._h, _p(info)), 'arp_poses_fingerprints_info')
        return dict(zip(('poses', 'n_refs', 'nodes', 'planes', 'words', 'slices', 'launches', 'flags'), (int(v) for v in info)))

    def poses_shortlist(self, kind, *, weights=None, ref=0, pose_ids=None, skip=0, k=None, min_score=None, tables=('atom_atom',),
                        sift_mask=0, ctype_mask=CTYPE_ALL):
        """The poses of the resident poses result (``poses_contacts`` / ``poses_summary``) ranked on the device and the chosen
        poses' records fetched, no other record copied (arp_poses_shortlist_*; ``arpeggio_amd.pose_shortlist``).  ``kind``:
        'summary' — score = ``weights`` (int32 [32], ``pose_shortlist.weights``) times the summary slots of the poses result
        and, second half, of the resident ``poses_planes`` result of the same poses; 'tanimoto' — the Tanimoto similarity (32
        fractional bits) to reference ``ref`` of the resident ``poses_fingerprints`` result, ``ref=-1`` the best over its
        references; 'list' — the poses ``pose_ids`` in that order.  Ranked are the poses from ``skip`` on, in descending score,
        ties by ascending pose id; chosen are the first ``k`` (default: all) with a score of at least ``min_score``.
        ``tables`` names what is fetched (``pose_shortlist.TABLES``); ``sift_mask`` / ``ctype_mask`` filter the records as
        ``contacts_filtered`` does (ring and amide records by ``ctype_mask``).  Returns a dict: ``pose`` int32 [K], ``score``
        int64 [K], ``summary`` uint32 [K, 16] (unfiltered), ``planes_summary`` when the planes result was read, ``movable``;
        for 'atom_atom' the five columns and ``pose_off`` — a ``poses`` table of K poses; per ring / amide table a dict
        shaped as ``poses_planes`` gives it."""
        from . import pose_shortlist as _sl, poses as _poses
        if kind not in _sl.KINDS:
            raise ValueError(f'poses_shortlist: kind must be one of {_sl.KINDS}')
        mask = _sl.tables_mask(tables)
        code = _sl.KINDS.index(kind)
        w = None if weights is None else np.ascontiguousarray(weights, np.int32).reshape(-1)
        if w is not None and len(w) != 32:
            raise ValueError('poses_shortlist: weights must be int32 [32] (pose_shortlist.weights)')
        ids = None if pose_ids is None else np.ascontiguousarray(pose_ids, np.int32).reshape(-1)
        if code == SHORTLIST_LIST:
            kk, ms = (0 if k is None else int(k)), (INT64_MIN if min_score is None else int(min_score))
        else:
            kk, ms = (POSES_MAX_POSES if k is None else int(k)), (INT64_MIN if min_score is None else int(min_score))
        info = np.zeros(8, np.int64)
        self._check(self._L.arp_poses_shortlist_launch(self._h, code, _p(w), int(ref), _p(ids), 0 if ids is None else len(ids), int(skip), kk, ms,
                                                       mask, int(sift_mask), int(ctype_mask), _p(info)), 'arp_poses_shortlist_launch')
        K = int(info[0])
        planes_read = (mask >> 1) != 0 or (code == SHORTLIST_SUMMARY and w is not None and bool(np.any(w[16:])))
        out = dict(pose=np.empty(K, np.int32), score=np.empty(K, np.int64), summary=np.empty((K, POSES_SUMMARY), np.uint32))
        if planes_read:
            out['planes_summary'] = np.empty((K, POSES_PLANES_SUMMARY), np.uint32)
        n, m = C.c_int64(0), C.c_int64(0)
        if mask & 1:
            kept = int(info[1])
            out.update(i=np.empty(kept, np.int32), j=np.empty(kept, np.int32), dist=np.empty(kept, np.float32), sift=np.empty(kept, np.uint16),
                       ctype=np.empty(kept, np.uint8), pose_off=np.empty(K + 1, np.uint64))
        else:
            kept = 0
        self._check(self._L.arp_poses_shortlist_fetch(self._h, K, kept, _p(out['pose']), _p(out['score']), _p(out['summary']),
                                                      _p(out.get('planes_summary')), _p(out.get('pose_off')), _p(out.get('i')), _p(out.get('j')),
                                                      _p(out.get('dist')), _p(out.get('sift')), _p(out.get('ctype')), C.byref(n), C.byref(m)),
                    'arp_poses_shortlist_fetch')
        for t, name in enumerate(_poses.PLANE_TABLES):
            if not (mask >> (t + 1)) & 1:
                continue
            kept = int(info[2 + t])
            tab, args = self._plane_table_buffers(name, kept, K + 1)
            self._check(self._L.arp_poses_shortlist_planes_fetch(self._h, t, K, kept, _p(tab['pose_off']), *args, C.byref(m)),
                        'arp_poses_shortlist_planes_fetch')
            out[name] = tab
        sel = getattr(self, '_sel', None)
        out['movable'] = np.nonzero(sel)[0].astype(np.int32) if sel is not None else np.zeros(0, np.int32)
        out['kind'] = kind
        return out

    def poses_shortlist_info(self):
        """arp_poses_shortlist_info: the chosen poses and the kept records per table of the resident shortlist (zeros while there
        is none), the launches that did work so far, and the kind."""
        from . import pose_shortlist as _sl
        info = np.zeros(8, np.int64)
        self._check(self._L.arp_poses_shortlist_info(self._h, _p(info)), 'arp_poses_shortlist_info')
        d = dict(chosen=int(info[0]))
        d.update({name: int(info[1 + t]) for t, name in enumerate(_sl.TABLES)})
        d.update(launches=int(info[6]), kind=int(info[7]))
        return d

    def poses_clusters(self, threshold_q32, *, order=None, skip=0, max_clusters=256):
        """Leader clustering of the poses of the resident fingerprint result (``poses_fingerprints``, either entry) by the Tanimoto
        similarity of their fingerprints, on the device (arp_poses_clusters_*; ``arpeggio_amd.pose_clusters``).  Position m names
        pose ``order[m]`` (int32 ids in [0, P), repeats allowed) or, without ``order``, pose ``skip + m``.  Walking the positions,
        a pose whose similarity (32 fractional bits) to some leader's pose reaches ``threshold_q32``
        (``pose_clusters.threshold_q32``) joins the FIRST such leader; otherwise it becomes the next leader while there are
        fewer than ``max_clusters`` (at most ``POSECL_MAX_CLUSTERS``), and stays unassigned after that.  Returns a dict: ``pose``
        int32 [M]; ``cluster`` int32 [M], -1 when unassigned; ``similarity`` int64 [M], to its own leader, 2^32 for a leader, -1
        when unassigned; ``leader`` int32 [C]; ``leader_position`` int32 [C]; ``size`` uint32 [C]; ``threshold_q32``,
        ``max_clusters``, ``unassigned``.  No record and no bit is copied."""
        ids = None if order is None else np.ascontiguousarray(order, np.int32).reshape(-1)
        info = np.zeros(8, np.int64)
        self._check(self._L.arp_poses_clusters_launch(self._h, _p(ids), 0 if ids is None else len(ids), int(skip), int(threshold_q32),
                                                      int(max_clusters), _p(info)), 'arp_poses_clusters_launch')
        M, Cn = int(info[0]), int(info[1])
        out = dict(pose=np.empty(M, np.int32), cluster=np.empty(M, np.int32), similarity=np.empty(M, np.int64), leader=np.empty(Cn, np.int32),
                   leader_position=np.empty(Cn, np.int32), size=np.empty(Cn, np.uint32))
        n, m = C.c_int64(0), C.c_int64(0)
        self._check(self._L.arp_poses_clusters_fetch(self._h, M, Cn, _p(out['pose']), _p(out['cluster']), _p(out['similarity']), _p(out['leader']),
                                                     _p(out['leader_position']), _p(out['size']), C.byref(n), C.byref(m)), 'arp_poses_clusters_fetch')
        out.update(threshold_q32=int(info[7]), max_clusters=int(info[3]), unassigned=int(info[2]))
        return out

    def poses_clusters_info(self):
        """arp_poses_clusters_info: positions, clusters, unassigned positions, ``max_clusters``, words per pose and the lanes per
        pose of the round kernel of the resident clusters (zeros while there are none), the launches that did work so far, and
        the threshold."""
        info = np.zeros(8, np.int64)
        self._check(self._L.arp_poses_clusters_info(self._h, _p(info)), 'arp_poses_clusters_info')
        return dict(zip(('positions', 'clusters', 'unassigned', 'max_clusters', 'words', 'lanes', 'launches', 'threshold_q32'), (int(v) for v in info)))

    # ---- a ligand library on the resident receptor (arp_library_*; ``arpeggio_amd.ligand_library``) ----
    def set_ligand_library(self, lib):
        """The ligand library beside the receptor (arp_set_ligand_library): ``lib`` as ``ligand_library.pack`` gives it.  It
        stays resident through new structures; a new library replaces it and voids the library result."""
        arr = dict(atom_off=np.ascontiguousarray(lib['atom_off'], np.int32), type_mask=np.ascontiguousarray(lib['type_mask'], np.uint16),
                   flags=np.ascontiguousarray(lib['flags'], np.uint16), vdw=np.ascontiguousarray(lib['vdw'], np.float64),
                   cov=np.ascontiguousarray(lib['cov'], np.float64), h_off=np.ascontiguousarray(lib['h_off'], np.int32),
                   sb_nbr=np.ascontiguousarray(lib['sb_nbr'], np.int32))
        L = len(arr['atom_off']) - 1
        if L < 1 or arr['atom_off'].ndim != 1:
            raise ValueError('set_ligand_library: atom_off must be [L + 1] with L >= 1')
        TA = int(arr['atom_off'][-1])
        # (the library reads TA entries of every per-atom array and TA + 1 offsets: their lengths are checked here)
        for k in ('type_mask', 'flags', 'vdw', 'cov', 'sb_nbr'):
            if arr[k].shape != (max(TA, 0),):
                raise ValueError(f'set_ligand_library: {k} must hold atom_off[-1] = {TA} entries')
        if arr['h_off'].shape != (max(TA, 0) + 1,):
            raise ValueError(f'set_ligand_library: h_off must hold atom_off[-1] + 1 = {TA + 1} entries')
        self._check(self._L.arp_set_ligand_library(self._h, L, _p(arr['atom_off']), _p(arr['type_mask']), _p(arr['flags']), _p(arr['vdw']),
                                                   _p(arr['cov']), _p(arr['h_off']), _p(arr['sb_nbr'])), 'arp_set_ligand_library')
        self._library = dict(atom_off=arr['atom_off'].astype(np.int64), h_off=arr['h_off'].astype(np.int64))

    def _library_launch(self, pose_off, xyz, h_xyz, cutoff, vdw_comp, include_sequence_adjacent):
        """Lengths checked against the resident library and ``pose_off``, then arp_library_contacts_launch; returns (T, records)."""
        lib = getattr(self, '_library', None)
        if lib is None:
            raise ValueError('library_contacts: no ligand library (set_ligand_library)')
        L = len(lib['atom_off']) - 1
        off = np.ascontiguousarray(pose_off, np.int64)
        if off.shape != (L + 1,):
            raise ValueError(f'library_contacts: pose_off must be [{L + 1}] (one entry per ligand of the library, and the total)')
        P = np.diff(off)
        S = np.diff(lib['atom_off'])
        SH = lib['h_off'][lib['atom_off'][1:]] - lib['h_off'][lib['atom_off'][:-1]]
        ok = off[0] == 0 and (P >= 0).all()
        nx, nh = (int((P * S).sum()) * 3, int((P * SH).sum()) * 3) if ok else (0, 0)
        x = np.ascontiguousarray(xyz, np.float32).reshape(-1)
        hx = np.zeros(0) if h_xyz is None else np.ascontiguousarray(h_xyz, np.float64).reshape(-1)
        if ok and len(x) != nx:
            raise ValueError(f'library_contacts: xyz must hold {nx} values (sum of P_l S_l 3, ligand-major then pose-major)')
        if ok and len(hx) != nh:
            raise ValueError(f'library_contacts: h_xyz must hold {nh} values (sum of P_l SH_l 3, ligand-major then pose-major)')
        n = C.c_int64(0)
        rc = self._L.arp_library_contacts_launch(self._h, _p(off), _p(x), _p(hx) if len(hx) else None, float(cutoff), float(vdw_comp),
                                                 int(bool(include_sequence_adjacent)), C.byref(n))
        try:
            self._check(rc, 'arp_library_contacts_launch')
        except NativeLibraryError as e:
            e.n_records = int(n.value)
            raise
        return int(off[-1]), int(n.value), off

    def library_contacts(self, pose_off, xyz, h_xyz, cutoff=5.0, vdw_comp=0.1, include_sequence_adjacent=False):
        """Every (ligand, pose)'s receptor - ligand contacts in one launch (arp_library_contacts_*).  ``pose_off`` int64 [L + 1]
        over the ligands of the resident library; ``xyz`` float32 and ``h_xyz`` float64, ligand-major then pose-major (flat or
        any shape of the right size; ``ligand_library.flatten_poses`` makes them).  Returns a dict: ``i`` (the receptor's packed
        id), ``a`` (the atom's index within its ligand), ``dist``, ``sift``, ``ctype`` in ascending (global pose, i, a),
        ``pose_off`` uint64 [T + 1], ``summary`` uint32 [T, 16] and ``ligand_pose_off`` int64 [L + 1] (the argument)."""
        T, k, off = self._library_launch(pose_off, xyz, h_xyz, cutoff, vdw_comp, include_sequence_adjacent)
        t = self._pose_records_fetch('arp_library_contacts_fetch', 'a', T, k)
        t['ligand_pose_off'] = off
        return t

    def library_summary(self, pose_off, xyz, h_xyz, cutoff=5.0, vdw_comp=0.1, include_sequence_adjacent=False):
        """``library_contacts`` with only the per-pose summary copied to the host: uint32 [T, 16]."""
        T, _, _ = self._library_launch(pose_off, xyz, h_xyz, cutoff, vdw_comp, include_sequence_adjacent)
        return self._pose_records_fetch('arp_library_contacts_fetch', None, T, 0)

    def library_best(self, weights):
        """The best pose of every ligand of the resident library result by ``weights`` int32 [16] over its summary row
        (arp_library_best_*): a dict of ``n_poses`` int64 [L], ``best_pose`` int32 [L] (global pose id, -1: the ligand has no
        pose) and ``score`` int64 [L] (INT64_MIN there).  20 bytes per ligand come back."""
        w = np.ascontiguousarray(weights, np.int64).reshape(-1)
        if w.shape != (POSES_SUMMARY,) or (np.abs(w) > SHORTLIST_MAX_WEIGHT).any():
            raise ValueError('library_best: weights must be 16 integers with |w| <= SHORTLIST_MAX_WEIGHT')
        w32 = w.astype(np.int32)
        self._check(self._L.arp_library_best_launch(self._h, _p(w32)), 'arp_library_best_launch')
        L = self.library_info()['ligands']
        out = dict(n_poses=np.empty(L, np.int64), best_pose=np.empty(L, np.int32), score=np.empty(L, np.int64))
        n = C.c_int64(0)
        self._check(self._L.arp_library_best_fetch(self._h, L, _p(out['n_poses']), _p(out['best_pose']), _p(out['score']), C.byref(n)),
                    'arp_library_best_fetch')
        return out

    def library_info(self):
        """arp_library_info: ligands, atoms, hydrogen rows and the largest ligand of the resident library; poses, records and
        the blocks of the launch of the resident result (zeros while there is none); whether a best-pose table is resident."""
        info = np.zeros(8, np.int64)
        self._check(self._L.arp_library_info(self._h, _p(info)), 'arp_library_info')
        return dict(ligands=int(info[0]), poses=int(info[1]), records=int(info[2]), atoms=int(info[3]), hydrogens=int(info[4]),
                    blocks=int(info[5]), max_atoms=int(info[6]), best=bool(info[7]))

    def set_ligand_library_planes(self, lib):
        """The plane table of the resident ligand library (arp_set_ligand_library_planes): the five arrays ``ring_off``,
        ``ring_atom_off``, ``ring_atom_idx``, ``amide_off`` and ``amide_atoms`` of ``lib`` as ``ligand_library.pack`` gives it — ring
        paths and amide atoms by index within the ligand.  It is dropped by ``set_ligand_library`` and replaced by a new call."""
        res = getattr(self, '_library', None)
        if res is None:
            raise ValueError('set_ligand_library_planes: no ligand library (set_ligand_library)')
        L = len(res['atom_off']) - 1
        arr = {k: np.ascontiguousarray(lib[k], np.int32) for k in ('ring_off', 'ring_atom_off', 'ring_atom_idx', 'amide_off')}
        am = np.ascontiguousarray(lib['amide_atoms'], np.int32).reshape(-1, 4)
        # (the library reads L + 1 offsets, ring_off[-1] + 1 ring offsets and as many indices and amides as those name: checked here)
        for k in ('ring_off', 'amide_off'):
            if arr[k].shape != (L + 1,):
                raise ValueError(f'set_ligand_library_planes: {k} must be [{L + 1}] (one entry per ligand of the library, and the total)')
        TR, TM = int(arr['ring_off'][-1]), int(arr['amide_off'][-1])
        if arr['ring_atom_off'].shape != (max(TR, 0) + 1,):
            raise ValueError(f'set_ligand_library_planes: ring_atom_off must hold ring_off[-1] + 1 = {TR + 1} entries')
        if arr['ring_atom_idx'].shape != (max(int(arr['ring_atom_off'][-1]), 0),):
            raise ValueError(f'set_ligand_library_planes: ring_atom_idx must hold ring_atom_off[-1] = {int(arr["ring_atom_off"][-1])} entries')
        if len(am) != max(TM, 0):
            raise ValueError(f'set_ligand_library_planes: amide_atoms must be [{TM}, 4]')
        self._check(self._L.arp_set_ligand_library_planes(self._h, _p(arr['ring_off']), _p(arr['ring_atom_off']),
                                                          _p(arr['ring_atom_idx']) if len(arr['ring_atom_idx']) else None, _p(arr['amide_off']),
                                                          _p(am) if len(am) else None), 'arp_set_ligand_library_planes')

    def _library_planes_launch(self, pose_off, xyz):
        """Lengths checked against the resident library and ``pose_off``, then arp_library_planes_launch; returns (T, counts, off)."""
        lib = getattr(self, '_library', None)
        if lib is None:
            raise ValueError('library_planes: no ligand library (set_ligand_library)')
        L = len(lib['atom_off']) - 1
        off = np.ascontiguousarray(pose_off, np.int64)
        if off.shape != (L + 1,):
            raise ValueError(f'library_planes: pose_off must be [{L + 1}] (one entry per ligand of the library, and the total)')
        P = np.diff(off)
        ok = off[0] == 0 and (P >= 0).all()
        nx = int((P * np.diff(lib['atom_off'])).sum()) * 3 if ok else 0
        x = np.ascontiguousarray(xyz, np.float32).reshape(-1)
        if ok and len(x) != nx:
            raise ValueError(f'library_planes: xyz must hold {nx} values (sum of P_l S_l 3, ligand-major then pose-major)')
        counts = np.zeros(4, np.int64)
        self._check(self._L.arp_library_planes_launch(self._h, _p(off), _p(x), _p(counts)), 'arp_library_planes_launch')
        return int(off[-1]), counts, off

    def library_planes(self, pose_off, xyz):
        """Every (ligand, pose)'s ring and amide contacts in one launch (arp_library_planes_*; ``arpeggio_amd.ligand_library``).
        ``pose_off`` int64 [L + 1] and ``xyz`` float32 as ``library_contacts`` takes them.  Returns a dict with one table per bag
        — ``atom_plane``, ``plane_plane``, ``group_group``, ``group_plane``: the columns of ``fetch_bag`` plus ``pose_off`` uint64
        [T + 1], per global pose exactly the records of the complex's bag that involve an affected entity, in the bag's canonical
        order, with the complex's ids (ligand atom n + a, ring n_rings + q, amide n_amides + g) —, ``summary`` uint32 [T, 16] and
        ``ligand_pose_off`` int64 [L + 1] (the argument)."""
        from . import poses as _poses
        T, counts, off = self._library_planes_launch(pose_off, xyz)
        out = {}
        n = C.c_int64(0)
        summary = np.empty((T, POSES_PLANES_SUMMARY), np.uint32)
        for t, name in enumerate(_poses.PLANE_TABLES):
            k = int(counts[t])
            tab, args = self._plane_table_buffers(name, k, T + 1)
            self._check(self._L.arp_library_planes_fetch(self._h, t, k, _p(tab['pose_off']), *args, _p(summary) if t == 0 else None, C.byref(n)),
                        'arp_library_planes_fetch')
            out[name] = tab
        out['summary'] = summary
        out['ligand_pose_off'] = off
        return out

    def library_planes_summary(self, pose_off, xyz):
        """``library_planes`` with only the per-pose summary copied to the host: uint32 [T, 16] (``poses.PLANE_SUMMARY_SLOTS``)."""
        T, _, _ = self._library_planes_launch(pose_off, xyz)
        s = np.empty((T, POSES_PLANES_SUMMARY), np.uint32)
        n = C.c_int64(0)
        self._check(self._L.arp_library_planes_fetch(self._h, 0, 0, *([None] * 10), _p(s), C.byref(n)), 'arp_library_planes_fetch')
        return s

    def library_planes_info(self):
        """arp_library_planes_info: ligands, rings and amides of the resident plane table; poses, records per table and the blocks
        of the launch of the resident result (zeros while there is none); the kernel launches so far; whether a plane table and
        the per-structure set-up are resident."""
        from . import poses as _poses
        info = np.zeros(12, np.int64)
        self._check(self._L.arp_library_planes_info(self._h, _p(info)), 'arp_library_planes_info')
        d = dict(ligands=int(info[0]), rings=int(info[1]), amides=int(info[2]), poses=int(info[3]))
        d.update({name: int(info[4 + t]) for t, name in enumerate(_poses.PLANE_TABLES)})
        d.update(blocks=int(info[8]), launches=int(info[9]), plane_table=bool(info[10]), setup=bool(info[11]))
        return d

    def library_fingerprints(self, refs, planes, ctype_mask=CTYPE_ALL, by_residue=True, bits=False):
        """The resident library result (``library_contacts`` / ``library_summary``) reduced on the device to interaction
        fingerprints and scored against reference interactions (arp_library_fingerprints_*; ``arpeggio_amd.library_fingerprints``).
        ``refs`` are the references as ``library_fingerprints.references`` gives them (``ref_off`` int64 [Q + 1], ``ref_node``
        int32 [F], ``ref_planes`` uint32 [F]; at most ``POSEFP_MAX_REFS``), or None for none: feature lists that need not come
        from poses of the launch.  A feature is (node, plane): the receptor residue (``by_residue=False``: receptor atom) of a
        record whose ``ctype`` bit is in ``ctype_mask``, and one of the SIFt bits of ``planes`` the record has.  Returns the
        dict ``poses_fingerprints`` returns, over Q + T rows — the references first, then the global poses: ``ids``, ``count``
        [Q + T], ``cross`` [Q + T, Q], ``occupancy`` [U, NP] over the poses, ``planes``, ``n_refs``, ``level``, with
        ``bits=True`` the bit matrix.  No record is copied.  Every call launches.

        A ``planes`` mask or a reference mask with a bit from ``POSEFP_PLANES`` on (``library_fingerprints.planes(classes=...)``,
        ``library_fingerprints.reference_from_plane_records``) adds the ring and amide classes as planes
        (arp_library_fingerprints_planes_launch): the resident ``library_planes`` result of the SAME poses is reduced into the
        same matrix, residue level only; ``planes`` in the result is the unified mask."""
        from . import library_fingerprints as _lfp
        r = _lfp.references([]) if refs is None else refs
        off = np.ascontiguousarray(r['ref_off'], np.int64).reshape(-1)
        node = np.ascontiguousarray(r['ref_node'], np.int32).reshape(-1)
        mask = np.ascontiguousarray(r['ref_planes'], np.uint32).reshape(-1)
        Q = len(off) - 1
        # (the library reads ref_off[Q] entries of both feature arrays: their lengths are checked here)
        if Q < 0 or len(node) != len(mask) or (Q > 0 and 0 <= int(off[-1]) != len(node)):
            raise ValueError('library_fingerprints: ref_node and ref_planes must hold ref_off[-1] entries each')
        flags = POSEFP_BY_RESIDUE if by_residue else 0
        info = np.zeros(8, np.int64)
        give = Q > 0
        wide = int(planes) >> POSEFP_PLANES or (len(mask) and int(mask.max()) >> POSEFP_PLANES)
        entry = 'arp_library_fingerprints_planes_launch' if wide else 'arp_library_fingerprints_launch'
        self._check(getattr(self._L, entry)(self._h, int(planes), int(ctype_mask), flags, Q, _p(off) if give else None,
                                            _p(node) if give else None, _p(mask) if give else None, _p(info)), entry)
        P, Q, U = (int(v) for v in info[:3])
        NP = bin(int(planes)).count('1')
        out = dict(ids=np.empty(U, np.int32), count=np.empty(P, np.uint32), cross=np.empty((P, Q), np.uint32), occupancy=np.empty((U, NP), np.uint32))
        if bits:
            out['bits'] = np.empty((P, NP, (U + 63) // 64), np.uint64)
        n = C.c_int64(0)
        self._check(self._L.arp_library_fingerprints_fetch(self._h, U, _p(out['ids']), _p(out['count']), _p(out['cross']), _p(out['occupancy']),
                                                           _p(out.get('bits')), C.byref(n)), 'arp_library_fingerprints_fetch')
        out.update(planes=int(planes), n_refs=Q, level='residue' if by_residue else 'atom')
        return out

    def library_fingerprints_best(self):
        """Per ligand and reference the best pose of the resident library fingerprint by Tanimoto similarity in 32 fractional
        bits (arp_library_fingerprints_best_*; ``library_fingerprints.best`` is the host mirror): a dict of ``n_poses`` int64
        [L], ``best_pose`` int32 [L, Q] (global pose id, ties to the lower one), ``tanimoto_q32`` int64 [L, Q], ``shared`` uint32
        [L, Q] and ``count`` uint32 [L, Q] (the best pose's own feature count).  A ligand without poses: -1, -1, 0, 0."""
        self._check(self._L.arp_library_fingerprints_best_launch(self._h), 'arp_library_fingerprints_best_launch')
        nl, nq = C.c_int64(0), C.c_int64(0)
        self._check(self._L.arp_library_fingerprints_best_fetch(self._h, 0, None, None, None, None, None, C.byref(nl), C.byref(nq)),
                    'arp_library_fingerprints_best_fetch')
        L, Q = int(nl.value), int(nq.value)
        out = dict(n_poses=np.empty(L, np.int64), best_pose=np.empty((L, Q), np.int32), tanimoto_q32=np.empty((L, Q), np.int64),
                   shared=np.empty((L, Q), np.uint32), count=np.empty((L, Q), np.uint32))
        self._check(self._L.arp_library_fingerprints_best_fetch(self._h, L, _p(out['n_poses']), _p(out['best_pose']), _p(out['tanimoto_q32']),
                                                                _p(out['shared']), _p(out['count']), C.byref(nl), C.byref(nq)),
                    'arp_library_fingerprints_best_fetch')
        return out

    def library_shortlist(self, kind, *, unit=None, weights=None, ref=0, pose_ids=None, k=None, min_score=None, tables=('atom_atom',),
                          sift_mask=0, ctype_mask=CTYPE_ALL):
        """The global poses of the resident library result (``library_contacts`` / ``library_summary``) — or, ``unit='ligands'``
        (the default of a ranked kind), its ligands, each by its best pose — ranked on the device and the chosen poses' records
        fetched, no other record copied (arp_library_shortlist_*; ``arpeggio_amd.library_shortlist``).  ``kind``: 'summary' —
        score = ``weights`` (int32 [32], ``library_shortlist.weights``) times the summary slots of the library result and,
        second half, of the resident ``library_planes`` result of the same poses; 'tanimoto' — the Tanimoto similarity (32
        fractional bits) to reference ``ref`` of the resident ``library_fingerprints`` result, ``ref=-1`` the best over its
        references; 'list' — the global poses ``pose_ids`` in that order (no ``unit``, ``k`` or ``min_score``).  Order:
        descending score, ties by ascending global pose; chosen are the first ``k`` (default: all) with a score of at least
        ``min_score``.  ``tables`` / ``sift_mask`` / ``ctype_mask`` as ``poses_shortlist``.  Returns a library table of K
        one-pose entries — ``i``, ``a``, ``dist``, ``sift``, ``ctype``, ``pose_off`` uint64 [K + 1] (for 'atom_atom'), ``summary``
        uint32 [K, 16], ``ligand_pose_off`` = 0 ... K (entry r stands where a ligand does: ``ligand_library.split`` works on it,
        ``library_shortlist.to_records`` names the real ligand) — with ``ligand`` int32 [K], ``pose`` int32 [K] (global pose),
        ``score`` int64 [K], ``planes_summary`` when the planes result was read, and per ring / amide table a dict shaped as
        ``library_planes`` gives it."""
        from . import pose_shortlist as _sl, poses as _poses
        if kind not in _sl.KINDS:
            raise ValueError(f'library_shortlist: kind must be one of {_sl.KINDS}')
        units = ('poses', 'ligands')
        code = _sl.KINDS.index(kind)
        if unit is None:
            unit = 'poses' if code == SHORTLIST_LIST else 'ligands'
        if unit not in units:
            raise ValueError(f'library_shortlist: unit must be one of {units}')
        mask = _sl.tables_mask(tables)
        w = None if weights is None else np.ascontiguousarray(weights, np.int32).reshape(-1)
        if w is not None and len(w) != 32:
            raise ValueError('library_shortlist: weights must be int32 [32] (library_shortlist.weights)')
        ids = None if pose_ids is None else np.ascontiguousarray(pose_ids, np.int32).reshape(-1)
        kk = (0 if code == SHORTLIST_LIST else POSES_MAX_POSES) if k is None else int(k)
        ms = INT64_MIN if min_score is None else int(min_score)
        info = np.zeros(8, np.int64)
        self._check(self._L.arp_library_shortlist_launch(self._h, code, units.index(unit), _p(w), int(ref), _p(ids), 0 if ids is None else len(ids),
                                                         kk, ms, mask, int(sift_mask), int(ctype_mask), _p(info)), 'arp_library_shortlist_launch')
        K = int(info[0])
        planes_read = (mask >> 1) != 0 or (code == SHORTLIST_SUMMARY and w is not None and bool(np.any(w[16:])))
        out = dict(ligand=np.empty(K, np.int32), pose=np.empty(K, np.int32), score=np.empty(K, np.int64),
                   summary=np.empty((K, POSES_SUMMARY), np.uint32))
        if planes_read:
            out['planes_summary'] = np.empty((K, POSES_PLANES_SUMMARY), np.uint32)
        n, m = C.c_int64(0), C.c_int64(0)
        kept = int(info[1]) if mask & 1 else 0
        if mask & 1:
            out.update(i=np.empty(kept, np.int32), a=np.empty(kept, np.int32), dist=np.empty(kept, np.float32), sift=np.empty(kept, np.uint16),
                       ctype=np.empty(kept, np.uint8), pose_off=np.empty(K + 1, np.uint64))
        self._check(self._L.arp_library_shortlist_fetch(self._h, K, kept, _p(out['ligand']), _p(out['pose']), _p(out['score']), _p(out['summary']),
                                                        _p(out.get('planes_summary')), _p(out.get('pose_off')), _p(out.get('i')), _p(out.get('a')),
                                                        _p(out.get('dist')), _p(out.get('sift')), _p(out.get('ctype')), C.byref(n), C.byref(m)),
                    'arp_library_shortlist_fetch')
        for t, name in enumerate(_poses.PLANE_TABLES):
            if not (mask >> (t + 1)) & 1:
                continue
            kept = int(info[2 + t])
            tab, args = self._plane_table_buffers(name, kept, K + 1)
            self._check(self._L.arp_library_shortlist_planes_fetch(self._h, t, K, kept, _p(tab['pose_off']), *args, C.byref(m)),
                        'arp_library_shortlist_planes_fetch')
            out[name] = tab
        out['ligand_pose_off'] = np.arange(K + 1, dtype=np.int64)
        out['kind'], out['unit'] = kind, unit
        return out

    def library_shortlist_info(self):
        """arp_library_shortlist_info: the chosen entries and the kept records per table of the resident library shortlist (zeros
        while there is none), the launches that did work so far, the kind and the unit."""
        from . import pose_shortlist as _sl
        info = np.zeros(8, np.int64)
        self._check(self._L.arp_library_shortlist_info(self._h, _p(info)), 'arp_library_shortlist_info')
        d = dict(chosen=int(info[0]))
        d.update({name: int(info[1 + t]) for t, name in enumerate(_sl.TABLES)})
        d.update(launches=int(info[6]), kind=int(info[7]) & 0xFF, unit=int(info[7]) >> 8)
        return d

    def library_clusters(self, threshold_q32, *, source='all', order=None, max_clusters=256):
        """Leader clustering of poses of the resident library result by the Tanimoto similarity of their library fingerprints
        (``library_fingerprints``, any references), on the device (arp_library_clusters_*; ``arpeggio_amd.library_clusters``).
        ``source``: 'all' — position m is global pose m; 'list' — global pose ``order[m]`` (int32 ids in [0, T), repeats
        allowed); 'shortlist' — the entries of the resident ``library_shortlist`` in rank order, read on the device.  Walking
        the positions, a pose whose similarity (32 fractional bits) to some leader's pose reaches ``threshold_q32``
        (``library_clusters.threshold_q32``) joins the FIRST such leader; otherwise it becomes the next leader while there are
        fewer than ``max_clusters`` (at most ``POSECL_MAX_CLUSTERS``), and stays unassigned after that.  Returns a dict:
        ``pose`` int32 [M] (global pose); ``ligand`` int32 [M]; ``cluster`` int32 [M], -1 when unassigned; ``similarity`` int64
        [M], to its own leader, 2^32 for a leader, -1 when unassigned; ``leader`` int32 [C]; ``leader_position`` int32 [C];
        ``size`` uint32 [C]; ``threshold_q32``, ``max_clusters``, ``unassigned``.  No record and no bit is copied."""
        sources = ('all', 'list', 'shortlist')
        if source not in sources:
            raise ValueError(f'library_clusters: source must be one of {sources}')
        ids = None if order is None else np.ascontiguousarray(order, np.int32).reshape(-1)
        info = np.zeros(8, np.int64)
        self._check(self._L.arp_library_clusters_launch(self._h, sources.index(source), _p(ids), 0 if ids is None else len(ids), int(threshold_q32),
                                                        int(max_clusters), _p(info)), 'arp_library_clusters_launch')
        M, Cn = int(info[0]), int(info[1])
        out = dict(pose=np.empty(M, np.int32), ligand=np.empty(M, np.int32), cluster=np.empty(M, np.int32), similarity=np.empty(M, np.int64),
                   leader=np.empty(Cn, np.int32), leader_position=np.empty(Cn, np.int32), size=np.empty(Cn, np.uint32))
        n, m = C.c_int64(0), C.c_int64(0)
        self._check(self._L.arp_library_clusters_fetch(self._h, M, Cn, _p(out['pose']), _p(out['ligand']), _p(out['cluster']), _p(out['similarity']),
                                                       _p(out['leader']), _p(out['leader_position']), _p(out['size']), C.byref(n), C.byref(m)),
                    'arp_library_clusters_fetch')
        out.update(threshold_q32=int(info[7]), max_clusters=int(info[3]), unassigned=int(info[2]))
        return out

    def library_clusters_info(self):
        """arp_library_clusters_info: positions, clusters, unassigned positions, ``max_clusters``, words per row and the rounds
        that elected a leader of the resident library clusters (zeros while there are none), the launches that did work so far,
        and the threshold."""
        info = np.zeros(8, np.int64)
        self._check(self._L.arp_library_clusters_info(self._h, _p(info)), 'arp_library_clusters_info')
        return dict(zip(('positions', 'clusters', 'unassigned', 'max_clusters', 'words', 'rounds', 'launches', 'threshold_q32'), (int(v) for v in info)))

    def library_water_bridges(self, contacts=('hbond', 'polar'), sift_any=None):
        """The ligand-water-receptor contacts of every pose of the resident library result, joined on the device with the atom-atom
        bag of a pass over the receptor alone, everything selected (arp_library_water_bridges_*; ``arpeggio_amd.library_bridges``
        describes the table).  ``contacts`` names the SIFt bits a leg needs one of (``library_bridges.mask``; ``None``: any), or
        ``sift_any`` gives the mask itself.  Returns a dict of the eight columns ``library_bridges.COLUMNS`` in ascending (pose,
        water, lig_atom, rec_atom) and, per pose, ``bridge_off`` uint64 [T + 1], ``waters`` uint32 [T] and ``legs`` uint32 [T].
        Only the table is copied to the host."""
        from . import library_bridges as _lb
        m = _lb.mask(contacts) if sift_any is None else int(sift_any)
        if m < 0 or m >= 1 << 32:
            raise ValueError('library_water_bridges: sift_any must fit 32 bits')
        n = C.c_int64(0)
        self._check(self._L.arp_library_water_bridges_launch(self._h, m, C.byref(n)), 'arp_library_water_bridges_launch')
        info = self.library_water_bridges_info()
        B, T = int(n.value), info['poses']
        out = {k: np.empty(B, dt) for k, dt in _lb.COLUMNS}
        out.update(bridge_off=np.empty(T + 1, np.uint64), waters=np.empty(T, np.uint32), legs=np.empty(T, np.uint32))
        # (the fetch writes B rows of every column and T + 1 / T / T per-pose entries: the arrays above are exactly that long)
        self._check(self._L.arp_library_water_bridges_fetch(self._h, B, T, *(_p(out[k]) for k, _ in _lb.COLUMNS), _p(out['bridge_off']),
                                                            _p(out['waters']), _p(out['legs']), C.byref(n)), 'arp_library_water_bridges_fetch')
        out['sift_any'] = m
        return out

    def library_water_bridges_info(self):
        """arp_library_water_bridges_info: poses, rows, ligand legs, receptor legs, waters with a receptor leg and the mask of the
        resident library water bridges (zeros while there are none), the launches that did work so far, and ``ready``: a library
        result and the atom-atom bag of a pass over the receptor with everything selected and the same cutoff and vdw_comp are
        resident, so a launch would not be refused for its sources."""
        info = np.zeros(8, np.int64)
        self._check(self._L.arp_library_water_bridges_info(self._h, _p(info)), 'arp_library_water_bridges_info')
        out = dict(zip(('poses', 'rows', 'ligand_legs', 'receptor_legs', 'receptor_waters', 'sift_any', 'launches'), (int(v) for v in info[:7])))
        out['ready'] = bool(info[7])
        return out

    def library_fingerprints_info(self):
        """arp_library_fingerprints_info: rows (references and poses), references, columns, planes, words per row and word slices
        of the resident library fingerprint (zeros while there is none), the launches so far, and the flags."""
        info = np.zeros(8, np.int64)
        self._check(self._L.arp_library_fingerprints_info(self._h, _p(info)), 'arp_library_fingerprints_info')
        return dict(zip(('rows', 'n_refs', 'nodes', 'planes', 'words', 'slices', 'launches', 'flags'), (int(v) for v in info)))

    def set_blob(self, blob, counts=None):
        """Upload a structure packed by ``pack_blob`` (one host-to-device copy); ``blob`` must stay alive during the call."""
        self._keep = blob
        self._models = None
        self._sel = None
        self._check(self._L.arp_set_blob(self._h, _p(blob), int(blob.nbytes)), 'arp_set_blob')
        hdr = BlobHeader.from_buffer_copy(blob[:C.sizeof(BlobHeader)].tobytes())
        self.n, self.n_rings, self.n_amides = int(hdr.n), int(hdr.nring), int(hdr.namide)

    def get_blob(self):
        """The resident structure read back in blob form (uint8 array; ``unpack_blob`` gives the arrays)."""
        nb = C.c_uint64()
        self._check(self._L.arp_get_blob(self._h, None, 0, C.byref(nb)), 'arp_get_blob')
        buf = np.empty(int(nb.value), np.uint8)
        self._check(self._L.arp_get_blob(self._h, _p(buf), int(buf.nbytes), C.byref(nb)), 'arp_get_blob')
        return buf

    # ---- exchange between shards: RCCL behind the C ABI (include/arpeggio_hip.h, arp_comm_*)
    @staticmethod
    def comm_unique_id():
        """128-byte id of a new communicator (rank 0 calls this and hands the bytes to the other ranks)."""
        buf = np.zeros(128, np.uint8)
        rc = load().arp_comm_unique_id(_p(buf), 128)
        if rc != ARP_OK:
            raise NativeLibraryError('arp_comm_unique_id failed: ' + load().arp_last_error(None).decode())
        return buf

    def comm_init(self, rank, world, unique_id):
        uid = np.ascontiguousarray(unique_id, np.uint8)
        if uid.size != 128:
            raise ValueError('the unique id has 128 bytes')
        self._check(self._L.arp_comm_init(self._h, int(rank), int(world), _p(uid)), 'arp_comm_init')
        self.comm_rank, self.comm_world = int(rank), int(world)

    def comm_info(self):
        """(rank, world) of the context's RCCL communicator as the library sees it (arp_comm_info)."""
        r, w = C.c_int(-1), C.c_int(0)
        self._check(self._L.arp_comm_info(self._h, C.byref(r), C.byref(w)), 'arp_comm_info')
        return int(r.value), int(w.value)

    def comm_destroy(self):
        self._check(self._L.arp_comm_destroy(self._h), 'arp_comm_destroy')

    def shard_exchange_faces(self, left, right):
        """``left`` / ``right``: (device pointer, bytes) from ``shard_pack_face`` or None.  Returns {-1: (ptr, bytes), +1: ...}
        of what the neighbours sent (buffers owned by the context)."""
        lp, lb = left if left else (0, 0)
        rp, rb = right if right else (0, 0)
        out = np.zeros(4, np.uint64)
        self._check(self._L.arp_shard_exchange_faces(self._h, lp, lb, rp, rb, _p(out)), 'arp_shard_exchange_faces')
        got = {}
        if out[1]:
            got[-1] = (int(out[0]), int(out[1]))
        if out[3]:
            got[+1] = (int(out[2]), int(out[3]))
        return got

    def shard_set_exchange_lists(self, send_left, send_right, recv_left, recv_right):
        a = [np.ascontiguousarray(x if x is not None else [], np.int32) for x in (send_left, send_right, recv_left, recv_right)]
        self._keep_lists = a
        self._check(self._L.arp_shard_set_exchange_lists(self._h, _p(a[0]), len(a[0]), _p(a[1]), len(a[1]), _p(a[2]), len(a[2]), _p(a[3]), len(a[3])),
                    'arp_shard_set_exchange_lists')

    def shard_exchange_plus(self):
        self._check(self._L.arp_shard_exchange_plus(self._h), 'arp_shard_exchange_plus')

    def shard_reduce_residue_sets(self):
        self._check(self._L.arp_shard_reduce_residue_sets(self._h), 'arp_shard_reduce_residue_sets')

    # ---- shard assembled on the device (sharding.make_shard_device)
    def shard_set_home(self, records):
        self._check(self._L.arp_shard_set_home(self._h, _p(records), int(records.nbytes)), 'arp_shard_set_home')

    def shard_pack_face(self, slot, x_lo, x_hi):
        """(device pointer, bytes) of the record buffer with the home items whose x lies in [x_lo, x_hi]."""
        ptr, nb = C.c_uint64(), C.c_uint64()
        self._check(self._L.arp_shard_pack_face(self._h, int(slot), float(x_lo), float(x_hi), C.byref(ptr), C.byref(nb)), 'arp_shard_pack_face')
        return int(ptr.value), int(nb.value)

    def shard_assemble(self, left, right, n_res_global):
        """``left`` / ``right``: (device pointer, bytes) of the halo buffers received from the neighbours, or None."""
        lp, lb = left[:2] if left else (0, 0)       # (a third element — the owner of the memory — is the caller's business)
        rp, rb = right[:2] if right else (0, 0)
        counts = np.zeros(3, np.int64)
        self._check(self._L.arp_shard_assemble(self._h, int(lp), int(lb), int(rp), int(rb), int(n_res_global), _p(counts)), 'arp_shard_assemble')
        self.n, self.n_rings, self.n_amides = int(counts[0]), int(counts[1]), int(counts[2])
        return counts

    def shard_layout(self):
        out = dict(global_id=np.empty(self.n, np.int32), origin=np.empty(self.n, np.int8), sel=np.empty(self.n, np.uint8),
                   ring_gid=np.empty(self.n_rings, np.int32), ring_origin=np.empty(self.n_rings, np.int8),
                   amide_gid=np.empty(self.n_amides, np.int32), amide_origin=np.empty(self.n_amides, np.int8))
        self._check(self._L.arp_shard_layout(self._h, *[_p(out[k]) for k in ('global_id', 'origin', 'sel', 'ring_gid', 'ring_origin',
                                                                              'amide_gid', 'amide_origin')]), 'arp_shard_layout')
        return out

    def set_ownership(self, is_home=None, global_id=None):
        home = None if is_home is None else np.ascontiguousarray(is_home, np.uint8)
        gid = None if global_id is None else np.ascontiguousarray(global_id, np.int32)
        self._check(self._L.arp_set_ownership(self._h, _p(home), _p(gid)), 'arp_set_ownership')

    def set_group_ownership(self, ring_home, ring_gid, amide_home, amide_gid):
        a = [np.ascontiguousarray(ring_home, np.uint8), np.ascontiguousarray(ring_gid, np.int32),
             np.ascontiguousarray(amide_home, np.uint8), np.ascontiguousarray(amide_gid, np.int32)]
        self._check(self._L.arp_set_group_ownership(self._h, *[_p(x) for x in a]), 'arp_set_group_ownership')

    def set_single_bond_neighbour_coords(self, sb_xyz, sb_present):
        x = np.ascontiguousarray(sb_xyz, np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(sb_present, np.uint8)
        self._check(self._L.arp_set_single_bond_neighbour_coords(self._h, _p(x), _p(f)), 'arp_set_single_bond_neighbour_coords')

    def set_selection_state(self, sel, plus, ring_sel, ring_plus, amide_sel, amide_plus):
        a = [np.ascontiguousarray(x, np.uint8) for x in (sel, plus, ring_sel, ring_plus, amide_sel, amide_plus)]
        self._check(self._L.arp_set_selection_state(self._h, *[_p(x) for x in a]), 'arp_set_selection_state')
        self._sel = None

    BUF_PLUS, BUF_RES_SETS, BUF_GRID_START, BUF_KEEP_BASE = 0, 1, 2, 3

    def device_buffer(self, which):
        """(device pointer, bytes) of a context buffer, for torch tensors that alias it (sharded runs)."""
        ptr, nb = C.c_uint64(0), C.c_int64(0)
        self._check(self._L.arp_device_buffer(self._h, int(which), C.byref(ptr), C.byref(nb)), 'arp_device_buffer')
        return int(ptr.value), int(nb.value)

    def run_stage(self, stage, cutoff=5.0, vdw_comp=0.1, include_sequence_adjacent=False, expand_radius=6.0):
        counts = np.zeros(5, np.int64)
        self._check(self._L.arp_run_stage(self._h, int(stage), float(cutoff), float(vdw_comp), int(bool(include_sequence_adjacent)),
                                          float(expand_radius), _p(counts)), 'arp_run_stage')
        return dict(atom_atom=int(counts[0]), plane_plane=int(counts[1]), atom_plane=int(counts[2]),
                    group_group=int(counts[3]), group_plane=int(counts[4]))

    def launch_bag(self, name):
        cnt = C.c_int64(0)
        self._check(getattr(self._L, f'arp_{name}_launch')(self._h, C.byref(cnt)), f'arp_{name}_launch')
        return int(cnt.value)

    # ---- searches ----
    def search_all(self, radius, active=None):
        act = None if active is None else np.ascontiguousarray(active, np.uint8)
        cap = max(16 * self.n, 1024)
        while True:
            oi, oj = np.empty(cap, np.int32), np.empty(cap, np.int32)
            cnt = C.c_int64(0)
            rc = self._L.arp_search_all(self._h, float(radius), _p(act), cap, _p(oi), _p(oj), C.byref(cnt))
            if rc == ARP_E_CAPACITY:
                cap = int(cnt.value)
                continue
            self._check(rc, 'arp_search_all')
            k = int(cnt.value)
            o = np.lexsort((oj[:k], oi[:k]))
            return oi[:k][o], oj[:k][o]

    def search(self, centers, radius):
        """``NeighborSearch.search(center, radius)`` for many centres: (centre index, atom index) of every atom within
        ``radius`` of a centre (all atoms, hydrogens included), sorted by centre then atom."""
        ctr = np.ascontiguousarray(centers, np.float64).reshape(-1, 3)
        cap = max(64 * len(ctr), 1024)
        while True:
            oc, oa = np.empty(cap, np.int32), np.empty(cap, np.int32)
            cnt = C.c_int64(0)
            rc = self._L.arp_search(self._h, float(radius), len(ctr), _p(ctr), cap, _p(oc), _p(oa), C.byref(cnt))
            if rc == ARP_E_CAPACITY:
                cap = int(cnt.value)
                continue
            self._check(rc, 'arp_search')
            k = int(cnt.value)
            return oc[:k].copy(), oa[:k].copy()

    def set_selection(self, in_selection):
        sel = np.ascontiguousarray(in_selection, np.uint8)
        if sel.shape != (self.n,):
            raise ValueError('in_selection must have one entry per atom')
        self._check(self._L.arp_set_selection(self._h, _p(sel)), 'arp_set_selection')
        self._sel = sel.copy()       # (the movable set of poses_contacts)

    def run_enqueue(self, cutoff=5.0, vdw_comp=0.1, include_sequence_adjacent=False, expand_radius=6.0):
        """First half of ``run_launch``: the pass is enqueued, the call returns.  Pair with ``run_wait``."""
        self._check(self._L.arp_run_enqueue(self._h, float(cutoff), float(vdw_comp), int(bool(include_sequence_adjacent)),
                                            float(expand_radius)), 'arp_run_enqueue')

    def run_wait(self):
        """Second half of ``run_launch``: waits for the enqueued pass, returns the five bag sizes."""
        rc = self._L.arp_run_wait(self._h, self._counts_p)
        if rc != ARP_OK:
            self._check(rc, 'arp_run_wait')
        c = self._counts
        return {'atom_atom': c[0], 'plane_plane': c[1], 'atom_plane': c[2], 'group_group': c[3], 'group_plane': c[4]}

    def run_launch(self, cutoff=5.0, vdw_comp=0.1, include_sequence_adjacent=False, expand_radius=6.0):
        """run_arpeggio on the resident structure; results stay in HBM.  Returns the five bag sizes."""
        rc = self._L.arp_run_launch(self._h, cutoff, vdw_comp, 1 if include_sequence_adjacent else 0, expand_radius, self._counts_p)
        if rc != ARP_OK:
            self._check(rc, 'arp_run_launch')
        c = self._counts
        return {'atom_atom': c[0], 'plane_plane': c[1], 'atom_plane': c[2], 'group_group': c[3], 'group_plane': c[4]}

    def make_selection_masks(self):
        """Masks computed by the last selection expansion (downloads only; no recomputation)."""
        L = self._L
        plus = np.empty(self.n, np.uint8)
        rs, rp = np.empty(self.n_rings, np.uint8), np.empty(self.n_rings, np.uint8)
        as_, ap = np.empty(self.n_amides, np.uint8), np.empty(self.n_amides, np.uint8)
        self._check(L.arp_get_selection(self._h, _p(plus), _p(rs), _p(rp), _p(as_), _p(ap)), 'arp_get_selection')
        return dict(plus=plus, ring_sel=rs, ring_plus=rp, amide_sel=as_, amide_plus=ap)

    def make_selection(self, in_selection=None, radius=6.0):
        sel = np.ones(self.n, np.uint8) if in_selection is None else np.ascontiguousarray(in_selection, np.uint8)
        if sel.shape != (self.n,):
            raise ValueError('in_selection must have one entry per atom')
        plus = np.empty(self.n, np.uint8)
        rs, rp = np.empty(self.n_rings, np.uint8), np.empty(self.n_rings, np.uint8)
        as_, ap = np.empty(self.n_amides, np.uint8), np.empty(self.n_amides, np.uint8)
        self._check(self._L.arp_make_selection(self._h, _p(sel), float(radius), _p(plus), _p(rs), _p(rp), _p(as_), _p(ap)),
                    'arp_make_selection')
        return dict(plus=plus, ring_sel=rs, ring_plus=rp, amide_sel=as_, amide_plus=ap)

    # ---- atom-atom contacts ----
    def atom_contacts_launch(self, cutoff=5.0, vdw_comp=0.1, include_sequence_adjacent=False):
        cnt = C.c_int64(0)
        self._check(self._L.arp_atom_contacts_launch(self._h, float(cutoff), float(vdw_comp), int(bool(include_sequence_adjacent)),
                                                     C.byref(cnt)), 'arp_atom_contacts_launch')
        return int(cnt.value)

    @staticmethod
    def pinned_contact_buffers(capacity):
        """Page-locked result buffers for ``atom_contacts_fetch(..., out=...)``: allocate once, reuse for every structure
        (the fetch then runs at PCIe speed; pinning memory costs more than one copy, so it is not done per call)."""
        cap = max(int(capacity), 1)
        return dict(i=pinned_empty(cap, np.int32), j=pinned_empty(cap, np.int32), dist=pinned_empty(cap, np.float32),
                    sift=pinned_empty(cap, np.uint16), ctype=pinned_empty(cap, np.uint8))

    def atom_contacts_fetch(self, count, sort=True, out=None):
        """Download the resident contact list.  ``out``: buffers from ``pinned_contact_buffers`` (the returned arrays
        are then views into them, valid until the next fetch into the same buffers)."""
        cap = max(int(count), 1)
        if out is not None and min(len(out[k]) for k in ('i', 'j', 'dist', 'sift', 'ctype')) >= cap:
            oi, oj, od, osf, oc = out['i'], out['j'], out['dist'], out['sift'], out['ctype']
            cap = min(len(a) for a in (oi, oj, od, osf, oc))
        else:
            oi, oj = np.empty(cap, np.int32), np.empty(cap, np.int32)
            od, osf, oc = np.empty(cap, np.float32), np.empty(cap, np.uint16), np.empty(cap, np.uint8)
        cnt = C.c_int64(0)
        if sort:      # canonical (i, j) order, made on the device (csrc/arp_sort.h)
            self._check(self._L.arp_atom_contacts_sort(self._h), 'arp_atom_contacts_sort')
        self._check(self._L.arp_atom_contacts_fetch(self._h, cap, _p(oi), _p(oj), _p(od), _p(osf), _p(oc), C.byref(cnt)),
                    'arp_atom_contacts_fetch')
        k = int(cnt.value)
        return dict(i=oi[:k], j=oj[:k], dist=od[:k], sift=osf[:k], ctype=oc[:k])

    def sort_contacts(self):
        """Put the resident atom-atom bag into the canonical (i, j) order (device radix sort; fetches after it deliver that order)."""
        self._check(self._L.arp_atom_contacts_sort(self._h), 'arp_atom_contacts_sort')

    # columns of the four ring / amide bags inside a packed fetch: (key, slot q of arp_fetch_packed's offsets, dtype)
    _PACKED_BAGS = tuple((name, tuple((key, q, dt) for key, dt, q in tables.bag_columns(name))) for name in tables.PACKED_ORDER)

    def fetch_packed(self, buf=None, sort_bags=True):
        """All five result bags of the last pass with ONE device-to-host copy (arp_fetch_packed): the atom-atom bag in
        canonical order (sorted on the device) and the ring / amide bags behind it.  ``buf``: a page-locked uint8 buffer
        from ``pinned_empty`` (reused from structure to structure; the returned arrays are views into it, valid until the
        next fetch into it); grown when too small.  Returns ``(bags, buf)``."""
        counts = (C.c_int64 * 5)()
        offs = (C.c_uint64 * 53)()
        used = C.c_uint64(0)
        if buf is None:
            buf = pinned_empty(1 << 20, np.uint8)
        rc = self._L.arp_fetch_packed(self._h, _p(buf), buf.nbytes, counts, offs, C.byref(used))
        if rc == ARP_E_CAPACITY and int(used.value) > buf.nbytes:
            buf = pinned_empty(int(used.value) + int(used.value) // 4 + 4096, np.uint8)
            rc = self._L.arp_fetch_packed(self._h, _p(buf), buf.nbytes, counts, offs, C.byref(used))
        if rc == ARP_E_CAPACITY and int(used.value) == 0:
            # a result too large for one piece (an array or the whole beyond 4 GiB): bag by bag, as before arp_fetch_packed
            # (counts[0]: what arp_fetch_packed filled before it failed — self._counts is only fresh after run_launch / run_wait)
            try:
                aa = self.atom_contacts_fetch(int(counts[0]), sort=True)
            except NativeLibraryError as e:
                if getattr(e, 'code', None) != ARP_E_CAPACITY:
                    raise
                # 2^31 records or more: beyond the device sort's tables — unsorted fetch, canonical order on the host
                aa = self.atom_contacts_fetch(int(counts[0]), sort=False)
                order = np.lexsort((aa['j'], aa['i']))
                aa = {k: v[order] for k, v in aa.items()}
            bags = {'atom_atom': aa}
            for name, _ in self._PACKED_BAGS:
                bags[name] = self.fetch_bag(name, sort=sort_bags)
            return bags, buf
        self._check(rc, 'arp_fetch_packed')
        return self._packed_views(buf, counts, offs), buf

    def _packed_views(self, buf, counts, offs):
        """The five bags of a packed fetch as views into ``buf`` (arp_fetch_packed's counts and offsets)."""
        def view(off, dtype, n):
            return np.frombuffer(buf, dtype, n, int(off)) if n else np.empty(0, dtype)
        k = int(counts[0])
        if getattr(self, '_packed_rows', False):
            bags = {'atom_atom': RowsBag(row=np.frombuffer(buf, np.int32, self.n + 1, int(offs[0])), j=view(offs[1], np.int32, k),
                                         dist=view(offs[2], np.float32, k), sift=view(offs[3], np.uint16, k), ctype=view(offs[4], np.uint8, k))}
        else:
            bags = {'atom_atom': dict(i=view(offs[0], np.int32, k), j=view(offs[1], np.int32, k), dist=view(offs[2], np.float32, k),
                                      sift=view(offs[3], np.uint16, k), ctype=view(offs[4], np.uint8, k))}
        for b, (name, cols) in enumerate(self._PACKED_BAGS):
            m = int(counts[1 + b])
            res = {key: view(offs[5 + 12 * b + q], dt, m) for key, q, dt in cols}
            # (every bag arrives in its canonical order, made on the device: one block's bitonic network for a bag of up to
            # BAG_SORT_MAX records, the radix passes of the atom-atom bag beyond that)
            bags[name] = res
        return bags

    def contacts_filter(self, sift_any=0x7FFF, ctype_mask=0x7F):
        """Filter the resident atom-atom bag of the last pass on the device (arp_contacts_filter_launch): a record is kept when
        ``(sift & sift_any) != 0`` and bit ``ctype`` of ``ctype_mask`` is set (``arpeggio_amd.contact_filter`` names the bits).
        The kept records are sorted into the canonical order there, in the layout ``set_packed_layout`` names; returns their
        number.  A second call with the same masks on the same results does no work."""
        kept = C.c_int64(0)
        self._check(self._L.arp_contacts_filter_launch(self._h, int(sift_any), int(ctype_mask), C.byref(kept)), 'arp_contacts_filter_launch')
        return int(kept.value)

    def fetch_packed_filtered(self, sift_any, ctype_mask=0x7F, buf=None):
        """``fetch_packed`` with the atom-atom bag filtered ON THE DEVICE first (``contacts_filter``, then
        arp_fetch_packed_filtered): only the kept records are sorted and cross PCIe, in canonical order — byte for byte the
        columns of ``fetch_packed`` masked with the predicate —, the four ring / amide bags complete behind them.  ``buf`` as
        in ``fetch_packed`` (grown when too small).  Returns ``(bags, buf)``; ``bags['atom_atom']`` is a ``RowsBag`` under the
        rows layout, ``bags['atom_atom_total']`` the unfiltered count."""
        self.contacts_filter(sift_any, ctype_mask)
        counts = (C.c_int64 * 5)()
        offs = (C.c_uint64 * 53)()
        used = C.c_uint64(0)
        if buf is None:
            buf = pinned_empty(1 << 20, np.uint8)
        rc = self._L.arp_fetch_packed_filtered(self._h, _p(buf), buf.nbytes, counts, offs, C.byref(used))
        if rc == ARP_E_CAPACITY and int(used.value) > buf.nbytes:
            buf = pinned_empty(int(used.value) + int(used.value) // 4 + 4096, np.uint8)
            rc = self._L.arp_fetch_packed_filtered(self._h, _p(buf), buf.nbytes, counts, offs, C.byref(used))
        self._check(rc, 'arp_fetch_packed_filtered')
        bags = self._packed_views(buf, counts, offs)
        bags['atom_atom_total'] = self.stats()['emitted']      # (arp_get_stats: the records the pass emitted)
        return bags, buf

    def atom_contacts(self, cutoff=5.0, vdw_comp=0.1, include_sequence_adjacent=False, sort=True):
        n = self.atom_contacts_launch(cutoff, vdw_comp, include_sequence_adjacent)
        out = self.atom_contacts_fetch(n, sort=sort)
        out['stats'] = self.stats()
        return out

    def atom_accumulators(self):
        """Per-atom sift masks (n,4) and hbond/polar counters (n,8) of the last contact launch."""
        sift = np.zeros((max(self.n, 1), 4), np.uint16)
        cnt = np.zeros((max(self.n, 1), 8), np.int32)
        self._check(self._L.arp_atom_accumulators(self._h, _p(sift), _p(cnt)), 'arp_atom_accumulators')
        return dict(sift=sift[:self.n], counts=cnt[:self.n])

    def atom_integer_sifts(self):
        """update_atom_integer_sift (U:224-242) under the canonical pair order: uint8 [n, 4, 15] =
        integer_sift / _inter_only / _intra_only / _water_only of the last contact launch."""
        out = np.zeros((max(self.n, 1), 4, 15), np.uint8)
        self._check(self._L.arp_atom_integer_sifts(self._h, _p(out)), 'arp_atom_integer_sifts')
        return out[:self.n]

    # ---- ring / amide contacts ----
    def pinned_bag_buffers(self, name, capacity):
        """Page-locked result buffers for ``fetch_bag(name, out=...)`` (allocate once, reuse for every structure)."""
        return tables.bag_buffers(name, max(int(capacity), 64), pinned_empty)

    def fetch_bag(self, name, sort=True, out=None):
        """Fetch one of the ring/amide bags left in HBM by run_launch (no re-computation).  ``out``: buffers from
        ``pinned_bag_buffers`` (the returned arrays are then views into them)."""
        fn = getattr(self._L, f'arp_{name}_fetch')
        mk, keys, order = self._BAGS[name]
        arrs = None
        if out is not None:
            cap, cnt = min(len(a) for a in out), C.c_int64(0)
            rc = fn(self._h, cap, *[_p(x) for x in out], C.byref(cnt))
            if rc == ARP_OK:
                arrs = [a[:int(cnt.value)] for a in out]
            elif rc != ARP_E_CAPACITY:
                self._check(rc, f'arp_{name}_fetch')
        if arrs is None:
            arrs = self._grow(lambda cap, r, cnt: fn(self._h, cap, *[_p(x) for x in r], C.byref(cnt)), mk, f'arp_{name}_fetch', 64)
        res = dict(zip(keys, arrs))
        if sort:
            o = np.lexsort((res[order[1]], res[order[0]]))
            res = {k: v[o] for k, v in res.items()}
        return res

    def _grow(self, call, arrays_factory, what, guess):
        cap = max(int(guess), 64)
        while True:
            arrs = arrays_factory(cap)
            cnt = C.c_int64(0)
            rc = call(cap, arrs, cnt)
            if rc == ARP_E_CAPACITY:
                cap = int(cnt.value)
                continue
            self._check(rc, what)
            k = int(cnt.value)
            return [a[:k] for a in arrs]

    def _bag_launch_fetch(self, name, guess):
        """Launch one ring / amide loop and fetch its bag in canonical order (arp_<name>)."""
        fn = getattr(self._L, f'arp_{name}')
        mk, keys, order = self._BAGS[name]
        a = self._grow(lambda cap, r, cnt: fn(self._h, cap, *[_p(x) for x in r], C.byref(cnt)), mk, f'arp_{name}', guess)
        out = dict(zip(keys, a))
        o = np.lexsort((out[order[1]], out[order[0]]))      # = the reference's creation order
        return {k: v[o] for k, v in out.items()}

    def atom_plane(self):
        return self._bag_launch_fetch('atom_plane', 8 * self.n_rings)

    def plane_plane(self):
        return self._bag_launch_fetch('plane_plane', 16 * self.n_rings)

    def group_group(self):
        return self._bag_launch_fetch('group_group', 8 * self.n_amides)

    def group_plane(self):
        return self._bag_launch_fetch('group_plane', 8 * self.n_amides)

    # per bag: (buffers for cap records, column names, sort keys) -- from tables.BAGS
    _BAGS = {name: ((lambda cap, name=name: tables.bag_buffers(name, cap)), tuple(c for c, _, _ in tables.bag_columns(name)), b.order)
             for name, b in tables.BAGS.items()}

    # ---- measurement ----
    def stats(self):
        s = np.zeros(8, np.int64)
        self._check(self._L.arp_get_stats(self._h, _p(s)), 'arp_get_stats')
        m = np.zeros(4, np.int64)
        self._check(self._L.arp_models_similarity_info(self._h, _p(m)), 'arp_models_similarity_info')
        lt = np.zeros(2, np.int64)
        self._check(self._L.arp_models_lifetimes_info(self._h, _p(lt)), 'arp_models_lifetimes_info')
        nw = np.zeros(3, np.int64)
        self._check(self._L.arp_networks_info(self._h, _p(nw)), 'arp_networks_info')
        cp = np.zeros(4, np.int64)
        self._check(self._L.arp_models_coupling_info(self._h, _p(cp)), 'arp_models_coupling_info')
        fp = np.zeros(8, np.int64)
        self._check(self._L.arp_poses_fingerprints_info(self._h, _p(fp)), 'arp_poses_fingerprints_info')
        cl = np.zeros(8, np.int64)
        self._check(self._L.arp_poses_clusters_info(self._h, _p(cl)), 'arp_poses_clusters_info')
        lc = np.zeros(8, np.int64)
        self._check(self._L.arp_library_clusters_info(self._h, _p(lc)), 'arp_library_clusters_info')
        return dict(candidates=int(s[0]), accepted=int(s[1]), emitted=int(s[2]), binned=int(s[3]), cells=int(s[4]),
                    expand_candidates=int(s[5]), expand_hits=int(s[6]), batch_restarts=int(s[7]),
                    sim_rows=int(m[0]), sim_words=int(m[1]), sim_slices=int(m[2]), sim_launches=int(m[3]),
                    posefp_nodes=int(fp[2]), posefp_words=int(fp[4]), posefp_slices=int(fp[5]), posefp_launches=int(fp[6]),
                    posecl_positions=int(cl[0]), posecl_clusters=int(cl[1]), posecl_launches=int(cl[6]),
                    libcl_positions=int(lc[0]), libcl_clusters=int(lc[1]), libcl_launches=int(lc[6]),
                    lifetimes_rows=int(lt[0]), lifetimes_launches=int(lt[1]),
                    couple_rows=int(cp[0]), couple_features=int(cp[1]), couple_tile_pairs=int(cp[2]), couple_launches=int(cp[3]),
                    networks_rows=int(nw[0]), networks_nodes=int(nw[1]), networks_launches=int(nw[2]))

    def set_profiling(self, on=True):
        self._check(self._L.arp_set_profiling(self._h, int(on)), 'arp_set_profiling')

    def kernel_times(self, reset=False):
        ms, ln = np.zeros(8, np.float64), np.zeros(8, np.int64)
        self._check(self._L.arp_get_kernel_times(self._h, _p(ms), _p(ln), int(reset)), 'arp_get_kernel_times')
        return {name: dict(ms=float(ms[k]), launches=int(ln[k])) for k, name in enumerate(KERNEL_SLOTS)}

    # ---- geometric part of initialize() (needs the atoms: set_complex / arp_set_atoms first) ----
    def ring_geometry(self, ring_atoms):
        """I:1697-1733: (center f64 [R,3], normal f64 [R,3]) of rings given as lists of atom indices in ring order."""
        nr = len(ring_atoms)
        off = np.zeros(nr + 1, np.int32)
        off[1:] = np.cumsum([len(a) for a in ring_atoms])
        idx = np.ascontiguousarray(np.concatenate([np.asarray(a, np.int32) for a in ring_atoms]) if nr else np.zeros(0, np.int32))
        ctr, nrm = np.zeros((max(nr, 1), 3), np.float64), np.zeros((max(nr, 1), 3), np.float64)
        self._check(self._L.arp_ring_geometry(self._h, nr, _p(off), _p(idx), _p(ctr), _p(nrm)), 'arp_ring_geometry')
        return ctr[:nr], nrm[:nr]

    def amide_geometry(self, amide_atoms):
        """I:1531-1589: (center f32 [A,3], normal f32 [A,3]) of amide groups given as [N, C, O, CA] atom indices."""
        at = np.ascontiguousarray(np.asarray(amide_atoms, np.int32).reshape(-1, 4))
        na = at.shape[0]
        ctr, nrm = np.zeros((max(na, 1), 3), np.float32), np.zeros((max(na, 1), 3), np.float32)
        self._check(self._L.arp_amide_geometry(self._h, na, _p(at), _p(ctr), _p(nrm)), 'arp_amide_geometry')
        return ctr[:na], nrm[:na]

    def ring_residues(self, ring_center):
        """I:1453-1492: (ring_res i32 [R], shortest distance f64 [R]) — residue of the nearest atom within 3.0 A, -1: none."""
        ctr = np.ascontiguousarray(np.asarray(ring_center, np.float64).reshape(-1, 3))
        nr = ctr.shape[0]
        res, dist = np.full(max(nr, 1), -1, np.int32), np.zeros(max(nr, 1), np.float64)
        self._check(self._L.arp_ring_residues(self._h, nr, _p(ctr), _p(res), _p(dist)), 'arp_ring_residues')
        return res[:nr], dist[:nr]

    def set_whole_structure(self, on=True):
        """Sharded runs without a selection: assert that the selection is the whole global structure (no exchange needed)."""
        self._check(self._L.arp_set_whole_structure(self._h, int(bool(on))), 'arp_set_whole_structure')

    def host_times(self, reset=False):
        """Per-pass host cost of run_launch: (enqueue_us, wait_us) averaged over the passes since the last reset."""
        us, n = np.zeros(2, np.float64), np.zeros(1, np.int64)
        self._check(self._L.arp_get_host_times(self._h, _p(us), _p(n), int(reset)), 'arp_get_host_times')
        k = max(int(n[0]), 1)
        return dict(enqueue_us=float(us[0]) / k, wait_us=float(us[1]) / k, passes=int(n[0]))

    def use_stream(self, stream_handle):
        self._check(self._L.arp_use_stream(self._h, int(stream_handle)), 'arp_use_stream')

    def stream_handle(self):
        return int(self._L.arp_stream_handle(self._h))
