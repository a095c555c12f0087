"""Host side of the residue-residue contact table (``Context.residue_pairs`` / ``InteractionComplex.residue_contacts`` /
``EnsembleComplex.run_residue_contacts``).

A table is a dict of seven NumPy columns, one row per unordered residue pair with at least one record in any of the five
bags of a pass, rows in ascending (res_a, res_b):

    res_a, res_b   int32        residue indices, res_a <= res_b
    n_contacts     uint32       atom-atom records of the pair
    dist_min       float32      smallest atom-atom distance of the pair (+inf when n_contacts == 0)
    bit_count      uint32 [15]  per SIFt bit (``config.SIFT_NAMES``): atom-atom records with it
    ctype_mask     uint8        OR of 1 << contact type over the atom-atom records
    plane_count    uint32 [4]   records of the atom-plane, plane-plane, group-group and group-plane bags (``PLANE_BAGS``)

Everything here is NumPy on the host: no GPU is needed to cut, label or export tables.
"""
import csv
import os

import numpy as np

from . import tables
from .core import config

COLUMNS = tables.RESPAIR.columns
N_BITS = tables.N_BITS
PLANE_BAGS = tables.PLANE_BAGS


def empty():
    """A table without rows."""
    return tables.empty(tables.RESPAIR)


def split(table, res_offsets):
    """The table of several structures resident at once, cut into one table per structure: ``res_offsets`` = the first
    residue index of every structure and, last, the resident residue count (a batch: ``off['residue']`` of
    ``batch.concat_complexes``; F models: ``np.arange(F + 1) * n_residues``).  No record joins two structures and the rows
    ascend by res_a, so structure s is the contiguous range of rows with res_a in [res_offsets[s], res_offsets[s + 1]) — a
    binary search, not a sort.  Residue ids come back structure-local."""
    off = np.asarray(res_offsets, np.int64)
    if off.ndim != 1 or len(off) < 1 or np.any(np.diff(off) < 0):
        raise ValueError('split: res_offsets must be ascending, one entry per structure and the total last')
    bounds = np.searchsorted(table['res_a'], off, side='left')
    out = []
    for s in range(len(off) - 1):
        lo, hi = int(bounds[s]), int(bounds[s + 1])
        t = {k: table[k][lo:hi] for k, _ in COLUMNS}
        if hi > lo and int(t['res_b'].max()) >= off[s + 1]:
            raise ValueError(f'split: a row of structure {s} reaches into the next one (res_offsets do not fit the table)')
        t['res_a'] = (t['res_a'] - off[s]).astype(np.int32)
        t['res_b'] = (t['res_b'] - off[s]).astype(np.int32)
        out.append(t)
    return out


def _residue_dict(lab, r):
    n, s, c, ic = lab.res_json[r]
    return {'label_comp_id': n, 'auth_seq_id': s, 'auth_asym_id': c, 'pdbx_PDB_ins_code': ic, 'label_comp_type': lab.res_comp_type[r]}


def to_records(table, pc, component_types=None):
    """The table as a list of dicts for JSON: 'bgn' / 'end' label the two residues with the keys ``get_contacts`` uses for a
    residue (export.py), the counts are plain ints, 'contact' maps each SIFt name that occurs to its number of atom-atom
    records, 'planes' each ring / amide bag that occurs to its number of records, 'interacting_entities' lists the contact
    types met, and 'distance_min' is None for a pair without atom-atom records."""
    from .core import export
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    out = []
    for r in range(len(table['res_a'])):
        n = int(table['n_contacts'][r])
        pl = table['plane_count'][r].tolist()
        out.append({'bgn': _residue_dict(lab, int(table['res_a'][r])), 'end': _residue_dict(lab, int(table['res_b'][r])),
                    'type': 'residue-residue', 'n_contacts': n, 'distance_min': float(table['dist_min'][r]) if n else None,
                    'contact': tables.sift_counts(table['bit_count'][r].tolist()),
                    'planes': {PLANE_BAGS[k]: pl[k] for k in range(len(PLANE_BAGS)) if pl[k]},
                    'interacting_entities': tables.contact_types(int(table['ctype_mask'][r]))})
    return out


CSV_HEADER = ['residue_bgn', 'residue_end', 'n_contacts', 'distance_min'] + list(config.SIFT_NAMES) + list(PLANE_BAGS) + \
             ['interacting_entities']


def write_csv(path, table, pc, component_types=None):
    """One row per residue pair: the residues in the form the other CSV tables use ('A/508/'), the number of atom-atom records
    and their smallest distance (empty without any), the fifteen SIFt counts, the four ring / amide counts and the contact
    types met, joined with '|'."""
    from .core import export
    lab = export.Labels(pc, pc.component_types if component_types is None else component_types)
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
        w.writerow(CSV_HEADER)
        for r in range(len(table['res_a'])):
            n = int(table['n_contacts'][r])
            w.writerow([lab.res_macro[int(table['res_a'][r])], lab.res_macro[int(table['res_b'][r])], n,
                        str(table['dist_min'][r]) if n else ''] + table['bit_count'][r].tolist() + table['plane_count'][r].tolist() +
                       ['|'.join(tables.contact_types(int(table['ctype_mask'][r])))])


def write_residue_contacts(wd, sid, table, pc, component_types=None):
    """'<id>.rescontacts' in ``wd``."""
    path = os.path.join(wd, sid + '.rescontacts')
    write_csv(path, table, pc, component_types)
    return path
