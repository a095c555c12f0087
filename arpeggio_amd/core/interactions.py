"""InteractionComplex — drop-in counterpart of ``arpeggio.core.InteractionComplex`` for the
``run_arpeggio`` / ``get_contacts`` path (reference: arpeggio/core/interactions.py:36-347, 2063-2113).

Same class name, method names, positional signatures and result attributes; the work is
done by the HIP library behind include/arpeggio_hip.h on a device-resident PackedComplex.
What the reference computes with BioPython/OpenBabel/gemmi before the hot path
(``__init__`` parsing and ``initialize()``'s typing, I:37-105, 288-327) is the *input
contract* here: the constructor takes a PackedComplex (or a ``.npz`` written by
``PackedComplex.save``); ``pack_from_reference_objects`` documents how a reference-side
object maps onto it.

There is no CPU fallback: without the HIP library and a GPU every compute method raises
NativeLibraryError.
"""
from __future__ import annotations

import collections
import logging
import os

import numpy as np

from . import config, export, utils
from .exceptions import AtomSerialError, NativeLibraryError
from .packed import PackedComplex

# result records: same field names as the reference (I:19-33); atoms / residues are packed indices
AtomPlaneContact = collections.namedtuple('AtomPlaneContact',
                                          ['bgn_atom', 'end_res', 'end_res_atoms', 'distance', 'sifts', 'text'])
PlanePlaneContact = collections.namedtuple('PlanePlaneContact',
                                           ['bgn_id', 'bgn_res', 'bgn_res_atoms', 'end_id', 'end_res', 'end_res_atoms',
                                            'distance', 'contact_type', 'text'])
AtomAtomContact = collections.namedtuple('AtomAtomContact', ['bgn_atom', 'end_atom', 'sifts', 'contact_type', 'distance'])
Parameters = collections.namedtuple('Parameters', ['vdw_comp_factor', 'interacting_threshold', 'has_hydrogens', 'ph'])


def ring_path_order(atoms, adj):
    """The atoms of one ring re-ordered so that consecutive ones (and the last and the first) are bonded: a walk over the
    bond graph ``adj`` (list of neighbour lists by packed index) restricted to the ring's atoms, from its first atom.
    Left as it is when the atoms do not form a single cycle in ``adj``."""
    atoms = [int(a) for a in atoms]
    members = set(atoms)
    path, seen = [atoms[0]], {atoms[0]}
    while len(path) < len(atoms):
        nxt = [b for b in adj[path[-1]] if b in members and b not in seen]
        if not nxt:
            return np.array(atoms, np.int32)
        path.append(int(nxt[0]))
        seen.add(path[-1])
    if path[0] not in adj[path[-1]]:
        return np.array(atoms, np.int32)
    return np.array(path, np.int32)


def amide_majority_residue(res_id, amide_atoms):
    """I:1554-1559: the residue of an amide group = ``max(residues, key=residues.count)`` over its four atoms N, C, O,
    C-alpha — the most frequent one, the FIRST such in that order on a tie."""
    r = np.asarray(res_id)[np.asarray(amide_atoms).reshape(-1, 4)]                     # [A, 4]
    cnt = (r[:, :, None] == r[:, None, :]).sum(axis=2)                                  # occurrences of each entry
    return r[np.arange(len(r)), cnt.argmax(axis=1)].astype(np.int32)                    # argmax: first maximum


class InteractionComplex:
    def __init__(self, filename, vdw_comp=0.1, interacting=5.0, ph=7.4, device=0, allow_incomplete=False):
        """Args mirror I:37.  ``filename``: the path of an mmCIF file (I:37-105 — read by ``core.protein_reader.read_mmcif``:
        what the file alone determines; see ``allow_incomplete``), a PackedComplex, or the path of a packed ``.npz``.
        ``allow_incomplete``: a structure read from a file lacks what only the reference's OpenBabel preparation gives
        (``pc.incomplete``); a run that needs a missing part raises ``IncompleteStructureError`` — with True it logs a warning
        and goes on (the records that depend on the missing part are then not the reference's)."""
        self.allow_incomplete = bool(allow_incomplete)
        if isinstance(filename, PackedComplex):
            self.pc = filename
            self.id = filename.id
        elif isinstance(filename, (str, os.PathLike)) and str(filename).endswith('.npz'):
            self.pc = PackedComplex.load(filename)
            self.id = os.path.basename(str(filename)).split('.')[0]        # I:51
        elif isinstance(filename, (str, os.PathLike)) and str(filename).lower().endswith(('.cif', '.mmcif')):
            from . import protein_reader
            self.pc = protein_reader.read_mmcif(str(filename))             # I:54-60, P:258-411
            self.id = os.path.basename(str(filename)).split('.')[0]        # I:51
        else:
            raise NotImplementedError(
                'Only mmCIF files (.cif), PackedComplex objects and packed .npz files are read: the reference converts every other '
                'format to mmCIF with gemmi first (P:258-295), which is outside the accelerated path.')
        self.pc.ensure_labels()
        self.device = device
        self._ctx = None
        self.component_types = self.pc.component_types                     # I:70

        # helper structures (I:73-81) — packed atom / ring / amide indices
        self.selection = []
        self.selection_ring_ids = []
        self.selection_amide_ids = []
        self.selection_plus = []
        self.selection_plus_residues = []
        self.selection_plus_ring_ids = []
        self.selection_plus_amide_ids = []
        # result bags (I:84-88)
        self._bags = {}
        self._contact_filter = None      # (sift_any, ctype_mask) of set_contact_filter
        self.params = Parameters(vdw_comp_factor=vdw_comp, interacting_threshold=interacting,
                                 has_hydrogens=bool(np.any(self.pc.flags & config.F_HYDROGEN)) or self.pc.h_xyz.shape[0] > 0,
                                 ph=ph)                                    # I:90-94

    # region public methods
    def structure_checks(self):
        """I:109-118."""
        serials = self.pc.serial
        if len(serials) > len(set(serials.tolist())):
            raise AtomSerialError

    def address_ambiguities(self):
        """I:120-133 strikes the ASN / GLN / HIS side-chain keys from four lists of the typing dictionary BEFORE initialize()
        types the atoms of standard residues from it (I:1966-1983).  Here the types are part of the packed input: the atoms of
        standard residues are re-typed from the same dictionary with those keys struck (``typing.apply_protein_typing``, pinned
        against the executed reference); every other atom keeps the types it was packed with."""
        from . import typing
        self.pc.type_mask = typing.apply_protein_typing(self.pc, use_ambiguities=True)
        if self._ctx is not None:
            self._ctx.set_complex(self.pc)

    def initialize(self):
        """I:288-327 prepares per-atom state; here: create the GPU context and upload the pack.  A structure that came from a
        file (``read_mmcif``) gets the centres / normals / residues of its template rings and amide groups computed on the GPU
        (the geometric part of I:1453-1492, 1531-1589, 1697-1733)."""
        from .. import _capi
        incomplete = getattr(self.pc, 'incomplete', ())
        if 'added hydrogens' in incomplete and not self.params.has_hydrogens and self.pc.n_atoms:
            # I:99-105: a structure without hydrogens gets them from OpenBabel (AddHydrogens at the given pH) — every hbond /
            # weak hbond flag depends on them
            self._incomplete(['hydrogens (the file has none; the reference adds them with OpenBabel, I:99-105)'])
        if self._ctx is None:
            self._ctx = _capi.Context(self.device)
            self._ctx.set_sort_after_pass(True)      # run_arpeggio always fetches the sorted bags next
        self._ctx.set_complex(self.pc)
        if getattr(self.pc, 'plane_geometry_pending', False):
            self.compute_plane_geometry()
            self.pc.plane_geometry_pending = False
        logging.debug('Uploaded packed structure to the GPU.')

    def _incomplete(self, needs):
        """A run on a structure read without OpenBabel needs something the file does not give."""
        from .exceptions import IncompleteStructureError
        if not self.allow_incomplete:
            raise IncompleteStructureError(needs)
        logging.warning('Structure read without OpenBabel, going on as asked (allow_incomplete); missing: %s', '; '.join(needs))

    def set_contact_filter(self, contacts=None, interacting_entities=None):
        """Extension beside the mirror (not in the reference): the next ``run_arpeggio`` fetches only the atom-atom records
        with at least one of the named ``contacts`` (``config.SIFT_NAMES``) between entities of one of the named
        ``interacting_entities`` kinds (``config.CONTACT_TYPE_NAMES``); ``None`` means all of that kind, and no arguments at
        all clear the filter.  The records are picked on the GPU before they are sorted and copied
        (``arpeggio_amd.contact_filter``, ``Context.fetch_packed_filtered``), so ``atom_contacts``, ``get_contacts``,
        ``write_json`` and ``write_contacts`` show the kept records only, the ring / amide bags whole.  What is made from the
        bag resident on the GPU does not change: ``atom_sifts``, ``atom_integer_sifts``, ``residue_sifts``,
        ``residue_contacts`` and the selection sets are those of the unfiltered run.  The check for what an incompletely read
        structure would have needed (``allow_incomplete``) looks at the records fetched, that is the kept ones."""
        from .. import contact_filter
        self._contact_filter = None if contacts is None and interacting_entities is None else contact_filter.masks(contacts, interacting_entities)

    def _check_incomplete_after_run(self):
        """What of ``pc.incomplete`` the run that has just finished would have needed: atom types, rings and amide groups of the
        non-standard residues inside selection_plus (OpenBabel's SMARTS and ring perception, I:1697-1733, 1531-1589, 1966-1983),
        and the single-bond neighbour of a halogen that takes part in a contact (U:139-141, 173).  It looks at the atom-atom
        records that were fetched: with ``set_contact_filter`` in force, the kept ones."""
        pc = self.pc
        incomplete = getattr(pc, 'incomplete', ())
        untyped = getattr(pc, 'untyped_atoms', None)
        if not incomplete or untyped is None or not len(untyped):
            return
        needs = []
        aa = self._bags.get('atom_atom', {})
        if len(aa.get('i', ())):
            hit = untyped[aa['i']] | untyped[aa['j']]
            if hit.any():
                res = sorted({pc.res_name[r].strip() for r in np.unique(pc.res_id[np.concatenate([aa['i'][hit], aa['j'][hit]])]).tolist()
                              if r in set(pc.res_id[untyped].tolist())})
                needs.append(f'atom types of the non-standard residues {", ".join(res[:8])} ({int(hit.sum())} of the contacts found touch '
                             f'their untyped atoms; also their rings and amide groups, if any)')
            hal = (pc.flags & config.F_HALOGEN) != 0
            if hal.any() and (hal[aa['i']] | hal[aa['j']]).any() and (pc.sb_nbr[hal] < 0).any():
                needs.append('bonds inside non-standard residues (the single-bond neighbour of a halogen in contact, U:139-141, 173)')
        if needs:
            self._incomplete(needs)

    def compute_plane_geometry(self, assign_ring_residues=True):
        """The geometric part of the reference's initialize() on the GPU, for packs that carry the perceived rings /
        amide groups only as atom lists (``ring_atoms``, ``amide_atoms``): ring centre + normal (I:1697-1733), amide
        centre + normal (I:1531-1589) and, if asked, the ring -> residue assignment by nearest atom (I:1453-1492).
        Overwrites ``ring_center / ring_normal / ring_res`` and ``amide_center / amide_normal`` of the pack and
        uploads them."""
        if self._ctx is None:
            self.initialize()
        pc, ctx = self.pc, self._ctx
        if pc.n_rings and pc.ring_atoms:
            # the normal is a sum of cross products of CONSECUTIVE centre->atom vectors (OBRing::findCenterAndNormal walks
            # the ring path): atoms listed in another order (e.g. file order CG, CD1, CD2, CE1, CE2, CZ) cancel to noise
            bad = pc.rings_not_in_path_order()
            if bad:
                raise ValueError(f'ring_atoms of ring(s) {bad[:8]} are not in ring-path order (consecutive atoms are not bonded): '
                                 'store the OpenBabel ring path, or keep the ring_center / ring_normal of the pack')
            pc.ring_center, pc.ring_normal = ctx.ring_geometry(pc.ring_atoms)
            if assign_ring_residues:
                pc.ring_res, self.ring_residue_shortest_distance = ctx.ring_residues(pc.ring_center)
        if pc.n_amides and (pc.amide_atoms[:, :3] >= 0).all():
            pc.amide_center, pc.amide_normal = ctx.amide_geometry(pc.amide_atoms)
            if (pc.amide_atoms >= 0).all():
                pc.amide_res = amide_majority_residue(pc.res_id, pc.amide_atoms)
        ctx.set_complex(pc)

    def run_arpeggio(self, user_selections, interacting_cutoff, vdw_comp, include_sequence_adjacent):
        """I:329-347: selection + binding-site expansion, atom, ring and amide contacts (all on the GPU)."""
        if self._ctx is None:
            self.initialize()
        pc, ctx = self.pc, self._ctx
        # I:1395: no selectors -> the whole structure.  Extension: an integer array = the packed indices of the
        # selected atoms (what the parser would have returned), for callers that select by their own means
        if isinstance(user_selections, np.ndarray):
            idx = np.unique(user_selections.astype(np.int64))
        elif user_selections:
            idx = utils.selection_parser(user_selections, pc)
        else:
            idx = np.arange(pc.n_atoms, dtype=np.int64)
        if idx.size == 0:                                                   # I:1399-1401
            logging.error('Selection was empty.')
            raise AttributeError('Selection must not be empty.')
        mask = np.zeros(pc.n_atoms, np.uint8)
        mask[idx] = 1
        ctx.set_selection(mask)
        counts = ctx.run_launch(interacting_cutoff, vdw_comp, include_sequence_adjacent,
                                config.SELECTION_EXPANSION_RADIUS)
        logging.debug('Completed new NeighbourSearch.')
        masks = ctx.make_selection_masks()
        self.selection = idx
        self.selection_plus = np.nonzero(masks['plus'])[0]
        self.selection_plus_residues = np.unique(pc.res_id[self.selection_plus])
        self.selection_ring_ids = set(np.nonzero(masks['ring_sel'])[0].tolist())
        self.selection_plus_ring_ids = set(np.nonzero(masks['ring_plus'])[0].tolist())
        self.selection_amide_ids = set(np.nonzero(masks['amide_sel'])[0].tolist())
        self.selection_plus_amide_ids = set(np.nonzero(masks['amide_plus'])[0].tolist())
        # all five bags with one copy; the atom-atom bag arrives in the canonical (i, j) order, made on the device
        # (the arrays are views into a page-locked buffer of their own: the next run allocates another one)
        if self._contact_filter is None:
            self._bags, _ = ctx.fetch_packed()
        else:      # (set_contact_filter: the kept atom-atom records only, picked on the device)
            self._bags, _ = ctx.fetch_packed_filtered(*self._contact_filter)
        self._check_incomplete_after_run()
        self.stats = ctx.stats()

    # ---- result bags as lists of the reference's namedtuples (built on demand) ----
    def _ring_names(self, r):
        return sorted(self.pc.atom_name[a] for a in self.pc.ring_atoms[r]) if self.pc.ring_atoms else []

    def _need_results(self):
        if 'atom_atom' not in self._bags:
            raise AttributeError('no results yet: call run_arpeggio() first')

    def _amide_names(self, a):
        return sorted(self.pc.atom_name[i] for i in self.pc.amide_atoms[a] if i >= 0)

    @property
    def atom_contacts(self):
        b = self._bags.get('atom_atom')
        if b is None:
            return []
        bits = {int(s): [(int(s) >> k) & 1 for k in range(15)] for s in np.unique(b['sift']).tolist()}
        with export.paused_gc():
            return [AtomAtomContact(i, j, list(bits[s]), config.CONTACT_TYPE_NAMES[c], d)
                    for i, j, s, c, d in zip(b['i'].tolist(), b['j'].tolist(), b['sift'].tolist(), b['ctype'].tolist(), b['dist'])]

    @property
    def plane_plane_contacts(self):
        b = self._bags.get('plane_plane')
        if b is None:
            return []
        out = []
        for k in range(len(b['bgn'])):
            types = [config.PLANE_PLANE_NAMES[b['type1'][k]]]
            if b['type2'][k] < config.PP_SAME:
                types.append(config.PLANE_PLANE_NAMES[b['type2'][k]])
            r1, r2 = int(b['bgn'][k]), int(b['end'][k])
            out.append(PlanePlaneContact(r1, int(self.pc.ring_res[r1]), self._ring_names(r1), r2, int(self.pc.ring_res[r2]),
                                         self._ring_names(r2), b['dist'][k], types, config.CONTACT_TYPE_NAMES[b['ctype'][k]]))
        return out

    @property
    def atom_plane_contacts(self):
        b = self._bags.get('atom_plane')
        if b is None:
            return []
        return [AtomPlaneContact(int(a), int(self.pc.ring_res[r]), self._ring_names(int(r)), d,
                                 [n for bit, n in enumerate(config.ATOM_PLANE_NAMES) if (int(m) >> bit) & 1],
                                 config.CONTACT_TYPE_NAMES[c])
                for a, r, d, m, c in zip(b['atom'], b['ring'], b['dist'], b['mask'], b['ctype'])]

    @property
    def group_group_contacts(self):
        b = self._bags.get('group_group')
        if b is None:
            return []
        return [PlanePlaneContact(int(a1), int(self.pc.amide_res[a1]), self._amide_names(int(a1)), int(a2),
                                  int(self.pc.amide_res[a2]), self._amide_names(int(a2)), d, ['AMIDEAMIDE'],
                                  config.CONTACT_TYPE_NAMES[c])
                for a1, a2, d, c in zip(b['bgn'], b['end'], b['dist'], b['ctype'])]

    @property
    def group_plane_contacts(self):
        b = self._bags.get('group_plane')
        if b is None:
            return []
        return [PlanePlaneContact(int(a), int(self.pc.amide_res[a]), self._amide_names(int(a)), int(r),
                                  int(self.pc.ring_res[r]), self._ring_names(int(r)), d, ['AMIDERING'],
                                  config.CONTACT_TYPE_NAMES[c])
                for a, r, d, c in zip(b['amide'], b['ring'], b['dist'], b['ctype'])]

    def residue_plane_sifts(self):
        """Per-residue integer SIFts of the ring / amide loops (I:1040-1057, 1171-1176, 1290-1291, 1371-1373).

        Returns int arrays indexed by residue: ``ring_ring_inter_integer_sift`` [NR,9] (FF..EF),
        ``ring_atom_inter_integer_sift`` / ``atom_ring_inter_integer_sift`` / ``mc_atom_ring_...`` / ``sc_atom_ring_...``
        [NR,5] (CARBONPI..METSULPHURPI), ``amide_amide_inter_integer_sift``, ``amide_ring_inter_integer_sift``,
        ``ring_amide_inter_integer_sift`` [NR,1].  Only contacts of type INTER between different residues count.
        """
        return residue_plane_sifts(self.pc, self._bags)

    # ---- per-atom / per-residue SIFt accumulators ----
    def atom_sifts(self):
        """Per-atom OR-accumulated SIFts of the last run (I:923-934, U:182-221), computed on the GPU from the resident
        contact list: dict of uint8 arrays [n_atoms, 15] ``sift``, ``sift_inter_only``, ``sift_intra_only``,
        ``sift_water_only`` and the int32 [n_atoms, 8] ``counts`` = actual hbonds {all, intra, inter, water} and actual
        polars {all, intra, inter, water} (I:821-852).  Rows of atoms outside ``selection_plus`` are zero."""
        acc = self._ctx.atom_accumulators()
        bits = (acc['sift'][:, :, None] >> np.arange(15, dtype=np.uint16)[None, None, :]) & 1
        names = ('sift', 'sift_inter_only', 'sift_intra_only', 'sift_water_only')
        out = {n: bits[:, k, :].astype(np.uint8) for k, n in enumerate(names)}
        out['counts'] = acc['counts']
        return out

    def atom_integer_sifts(self):
        """``atom.integer_sift`` / ``_inter_only`` / ``_intra_only`` / ``_water_only`` (U:224-242, called at I:924-925) as
        a uint8 array [n_atoms, 4, 15].  The reference's values are decided by the last pair its KD-tree delivers for each
        atom; here the delivery order is the canonical one (contacts sorted by (bgn, end)), see include/arpeggio_hip.h."""
        self._need_results()
        return self._ctx.atom_integer_sifts()

    def residue_sifts(self):
        """`_calc_residue_sifts` (I:471-574): dict name -> int array [n_residues, width] with the reference's attribute
        names (``sift``, ``mc_sift_inter_only``, ``integer_sift``, ``ring_ring_inter_integer_sift`` ...), in the column
        order of `write_residue_sifts`."""
        self._need_results()
        bits = self.atom_sifts()
        return export.residue_sift_table(self.pc, bits, self.atom_integer_sifts(), self.residue_plane_sifts())

    def residue_contacts(self):
        """The residue-residue contact table of the last run (``arpeggio_amd.residue_pairs`` describes the seven columns): the
        records of all five bags folded by residue on the GPU, from the results ``run_arpeggio`` left resident there — only
        the table is copied."""
        self._need_results()
        if self._ctx is None:
            raise AttributeError('no results on a GPU context: call run_arpeggio() on this complex first')
        return self._ctx.residue_pairs()

    def write_residue_contacts(self, wd):
        """'<id>.rescontacts': ``residue_contacts()`` as CSV, one row per residue pair (``residue_pairs.write_csv``)."""
        from .. import residue_pairs
        return residue_pairs.write_residue_contacts(wd, self.id, self.residue_contacts(), self.pc, self.component_types)

    def water_bridges(self, contacts=('hbond', 'polar'), same_residue=False):
        """Extension beside the mirror (not in the reference, which marks water contacts — I:643-691, 821-852 — but never says
        what a water sits between): the water-mediated contacts of the last run, one row per water and unordered pair of the
        atoms it touches through a record with one of the named ``contacts`` (``config.SIFT_NAMES``; ``None``: any); pairs of
        one residue only with ``same_residue``.  ``arpeggio_amd.water_bridges`` describes the nine columns.  The atom-atom bag
        that ``run_arpeggio`` left resident on the GPU is joined with itself there — only the table is copied — whatever
        ``set_contact_filter`` made of the fetched records."""
        from .. import water_bridges as wb
        self._need_results()
        if self._ctx is None:
            raise AttributeError('no results on a GPU context: call run_arpeggio() on this complex first')
        return self._ctx.water_bridges(wb.mask(contacts), wb.SAME_RESIDUE if same_residue else 0)

    def write_water_bridges(self, wd, contacts=('hbond', 'polar'), same_residue=False):
        """'<id>.waterbridges': ``water_bridges()`` as CSV, one row per bridge with the atom labels of the other CSV writers
        (``water_bridges.write_csv``)."""
        from .. import water_bridges as wb
        return wb.write_water_bridges(wd, self.id, self.water_bridges(contacts, same_residue), self.pc, self.component_types)

    def networks(self, contacts=None, interacting_entities=None, level='atom'):
        """Extension beside the mirror (the reference has no graph view of its contacts): the interaction networks of the last
        run — the connected components of the graph whose nodes are the atoms (``level='atom'``) or the residues
        (``'residue'``) and whose edges are the atom-atom records with one of the named ``contacts`` between the named
        ``interacting_entities`` (``contact_filter.masks``; ``None``: all).  Returns ``(label, table)``: per node the smallest
        node id of its component or -1 without such a record, and one row per component (``arpeggio_amd.networks`` describes
        both).  The ring and amide bags take no part.  The atom-atom bag that ``run_arpeggio`` left resident on the GPU is
        read there — only the labels and the table are copied — whatever ``set_contact_filter`` made of the fetched records."""
        from .. import contact_filter
        if level not in ('atom', 'residue'):
            raise ValueError("networks: level must be 'atom' or 'residue'")
        sift_any, ctype_mask = contact_filter.masks(contacts, interacting_entities)
        self._need_results()
        if self._ctx is None:
            raise AttributeError('no results on a GPU context: call run_arpeggio() on this complex first')
        return self._ctx.networks(sift_any, ctype_mask, level == 'residue')

    def write_networks(self, wd, contacts=None, interacting_entities=None, level='atom'):
        """'<id>.networks': ``networks()`` as CSV, one row per component with its members in the atom / residue labels of the
        other CSV writers (``networks.write_csv``)."""
        from .. import networks as nw
        label, table = self.networks(contacts, interacting_entities, level)
        return nw.write_networks(wd, self.id, label, table, self.pc, level, self.component_types)

    def run_poses(self, user_selections, xyz, h_xyz, interacting_cutoff, vdw_comp, include_sequence_adjacent, chunk=None, planes=False):
        """Extension beside the mirror (the reference evaluates one placement per run): the contacts of many poses of a ligand
        against this structure as the fixed receptor.  ``user_selections`` names the ligand, the MOVABLE SET (selectors, or
        an integer array of packed atom ids); ``xyz`` float32 [P, S, 3] are its atoms' coordinates per pose in ascending packed
        order and ``h_xyz`` float64 [P, SH, 3] the hydrogen rows of those atoms (``arpeggio_amd.poses.movable`` lists both).
        Per pose the result holds exactly the atom-atom records between the ligand and the rest that ``run_arpeggio`` would
        find on the structure with the pose scattered in — computed on the GPU against the resident receptor, only the poses
        uploaded.  Returns the table ``arpeggio_amd.poses`` describes (also kept in ``self.poses``); the poses go to the device
        ``chunk`` at a time (default: all at once, at most ``_capi.POSES_MAX_POSES``).  ``interacting_cutoff`` <= 6.0.  The
        results of the last ``run_arpeggio`` stay as they are, but the selection on the device is the ligand from here on.
        ``planes=True``: the ring and amide contacts of every pose as well (``Context.poses_planes``; the pack needs
        ``ring_atoms`` and ``amide_atoms``), kept in ``self.pose_planes`` (``poses.concat_planes`` over the chunks)."""
        from .. import _capi, poses as _poses
        if self._ctx is None:
            self.initialize()
        pc, ctx = self.pc, self._ctx
        if isinstance(user_selections, np.ndarray):
            idx = np.unique(user_selections.astype(np.int64))
        else:
            idx = utils.selection_parser(user_selections, pc) if user_selections else np.zeros(0, np.int64)
        if idx.size == 0:
            raise AttributeError('Selection must not be empty.')
        mask = np.zeros(pc.n_atoms, np.uint8)
        mask[idx] = 1
        ctx.set_selection(mask)
        x = np.ascontiguousarray(xyz, np.float32)
        h = None if h_xyz is None else np.ascontiguousarray(h_xyz, np.float64)
        step = int(chunk) if chunk else min(max(len(x), 1), _capi.POSES_MAX_POSES)
        parts = [ctx.poses_contacts(x[a:a + step], None if h is None else h[a:a + step], interacting_cutoff, vdw_comp, include_sequence_adjacent)
                 for a in range(0, len(x), step)]
        if not parts:
            raise ValueError('run_poses: no pose given')
        self.poses = parts[0] if len(parts) == 1 else _poses.concat(parts)
        if planes:
            ctx.set_plane_atoms(pc)
            pparts = [ctx.poses_planes(x[a:a + step]) for a in range(0, len(x), step)]
            self.pose_planes = pparts[0] if len(pparts) == 1 else _poses.concat_planes(pparts)
        return self.poses

    def write_poses(self, wd):
        """'<id>.poses': the table of the last ``run_poses`` as CSV, one row per record (``poses.write_csv``)."""
        from .. import poses as _poses
        if getattr(self, 'poses', None) is None:
            raise AttributeError('no poses yet: call run_poses() first')
        return _poses.write_poses(wd, self.id, self.poses, self.pc, self.component_types)

    def run_ligand_library(self, ligands, poses, interacting_cutoff, vdw_comp, include_sequence_adjacent, chunk=None, weights=None, planes=False):
        """Extension beside the mirror: the contacts of many DIFFERENT ligands, each with its poses, against this structure as
        the fixed receptor (``arpeggio_amd.ligand_library``; ``run_poses`` moves one ligand that is part of the structure).
        ``ligands`` are packs of one residue each (``ligand_library.pack`` says what is refused); ``poses`` holds per ligand
        ``(xyz float32 [P_l, S_l, 3], h_xyz float64 [P_l, SH_l, 3] or None)``, or None for a ligand without poses.  Per (ligand,
        pose) the result holds exactly the atom-atom records between the receptor and the ligand that ``run_arpeggio`` would find
        on the receptor with the ligand appended as one more residue and selected.  The receptor is uploaded once and the library
        once; ``chunk`` cuts the launches by total poses (default: all at once, at most ``_capi.POSES_MAX_POSES``; a ligand's
        poses may be cut between two launches).  Returns the table ``ligand_library`` describes (kept in ``self.ligand_library``,
        the ligands in ``self.ligand_library_ligands``).  ``weights`` int [16]: also the best pose per ligand by the weighted sum
        of its summary row (``self.ligand_library_best``): from the device when one launch held every pose, else the host mirror
        over the joined summaries.  ``planes``: every chunk is also launched as ``Context.library_planes`` — the ring and amide
        contacts of the same poses, from the ligands' ``ring_atoms`` / ``amide_atoms`` —, kept in ``self.library_planes``
        (``ligand_library.concat_planes`` over the chunks; None after a run without ``planes``).  The results of the last ``run_arpeggio`` and of ``run_poses`` stay as
        they are."""
        from .. import _capi, ligand_library as _ll
        if self._ctx is None:
            self.initialize()
        ctx = self._ctx
        ligands = list(ligands)
        lib = _ll.pack(ligands)
        off, x, h = _ll.flatten_poses(lib, poses)
        if off[-1] < 1:
            raise ValueError('run_ligand_library: no pose given')
        ctx.set_ligand_library(lib)
        if planes:
            ctx.set_ligand_library_planes(lib)
        parts, plane_parts = [], []
        for off_c, _, _, xc, hc in _ll.chunk_poses(lib, off, x, h, chunk if chunk else _capi.POSES_MAX_POSES):
            parts.append(ctx.library_contacts(off_c, xc, hc, interacting_cutoff, vdw_comp, include_sequence_adjacent))
            if planes:
                plane_parts.append(ctx.library_planes(off_c, xc))
        self.ligand_library = parts[0] if len(parts) == 1 else _ll.concat(parts)
        # (without planes an earlier planes result is dropped: it belongs to the ligands of that run)
        self.library_planes = None if not planes else plane_parts[0] if len(plane_parts) == 1 else _ll.concat_planes(plane_parts)
        self.ligand_library_ligands = ligands
        if weights is not None:
            self.ligand_library_best = ctx.library_best(weights) if len(parts) == 1 else _ll.best(self.ligand_library, weights)
        return self.ligand_library

    def write_ligand_library(self, wd):
        """'<id>.library': the table of the last ``run_ligand_library`` as CSV, one row per record (``ligand_library.write_csv``)."""
        from .. import ligand_library as _ll
        if getattr(self, 'ligand_library', None) is None:
            raise AttributeError('no ligand library result yet: call run_ligand_library() first')
        return _ll.write_library(wd, self.id, self.ligand_library, self.pc, self.ligand_library_ligands, self.component_types)

    def run_library_water_bridges(self, library, poses, contacts=('hbond', 'polar'), chunk=None, interacting_cutoff=5.0, vdw_comp=0.1):
        """Extension beside the mirror: which ligand atom of which pose is tied to which receptor atom through which structural
        water, joined ON THE DEVICE (``arpeggio_amd.library_bridges`` describes the table).  ``library`` is a list of ligand packs
        and ``poses`` holds per ligand ``(xyz, h_xyz or None)`` or None, as ``run_ligand_library`` takes them; ``contacts`` names the
        SIFt bits a leg needs one of (``None``: any).  The atom-atom bag of a pass over this structure alone with everything
        selected is the second source: when none with the same ``interacting_cutoff`` and ``vdw_comp`` is resident, that pass is
        run here first (the selection on the device is everything from then on).  Every chunk of ``chunk`` global poses (default:
        all at once; a ligand's poses may be cut between two) is one ``Context.library_summary`` and one
        ``Context.library_water_bridges``; the chunks are joined by global pose (``library_bridges.concat``).  Returns the table,
        with ``ligand_pose_off``; also kept in ``self.library_water_bridges`` (the ligands in ``self.library_water_bridges_ligands``)."""
        from .. import _capi, ligand_library as _ll, library_bridges as _lb
        sift_any = _lb.mask(contacts)
        if self._ctx is None:
            self.initialize()
        ctx = self._ctx
        ligands = list(library)
        lib = _ll.pack(ligands)
        off, x, h = _ll.flatten_poses(lib, poses)
        if off[-1] < 1:
            raise ValueError('run_library_water_bridges: no pose given')
        ctx.set_ligand_library(lib)
        parts = []
        for off_c, _, _, xc, hc in _ll.chunk_poses(lib, off, x, h, chunk if chunk else _capi.POSES_MAX_POSES):
            ctx.library_summary(off_c, xc, hc, interacting_cutoff, vdw_comp, False)
            if not ctx.library_water_bridges_info()['ready']:
                # no bag of a pass over the whole receptor with these parameters is resident: that pass, once (it voids no library result)
                ctx.set_selection(np.ones(self.pc.n_atoms, np.uint8))
                ctx.atom_contacts_launch(interacting_cutoff, vdw_comp, False)
            parts.append(ctx.library_water_bridges(sift_any=sift_any))
        out = parts[0] if len(parts) == 1 else _lb.concat(parts)
        out['ligand_pose_off'] = off
        self.library_water_bridges = out
        self.library_water_bridges_ligands = ligands
        return out

    def write_library_water_bridges(self, wd):
        """'<id>.librarybridges': the table of the last ``run_library_water_bridges`` as CSV, one row per bridge
        (``library_bridges.write_csv``)."""
        from .. import library_bridges as _lb
        t = getattr(self, 'library_water_bridges', None)
        if t is None:
            raise AttributeError('no library water bridges yet: call run_library_water_bridges() first')
        return _lb.write_library_bridges(wd, self.id, t, self.pc, self.library_water_bridges_ligands, t['ligand_pose_off'], self.component_types)

    def write_library_planes(self, wd):
        """'<id>.libraryplanes': the ring and amide table of the last ``run_ligand_library(planes=True)`` as CSV, one row per record
        (``ligand_library.write_planes_csv``)."""
        from .. import ligand_library as _ll
        if getattr(self, 'library_planes', None) is None:
            raise AttributeError('no library planes result yet: call run_ligand_library(planes=True) first')
        return _ll.write_library_planes(wd, self.id, self.library_planes, self.pc, self.ligand_library_ligands, self.component_types)

    def run_library_fingerprints(self, library, pose_off, xyz, h_xyz, refs, contacts=None, interacting_entities=None, level='residue',
                                 chunk=None, interacting_cutoff=5.0, vdw_comp=0.1, classes=()):
        """Extension beside the mirror: which ligands of a library reproduce the interactions of known binders, scored ON THE
        DEVICE — no record is copied (``arpeggio_amd.library_fingerprints``).  ``library`` is a list of ligand packs or what
        ``ligand_library.pack`` made of one; ``pose_off`` int64 [L + 1], ``xyz`` and ``h_xyz`` are the flat arrays of
        ``ligand_library.flatten_poses``.  ``refs`` are the references as ``library_fingerprints.references`` gives or takes
        them: feature lists at ``level`` ('residue' or 'atom') that need not come from poses of this library
        (``library_fingerprints.reference_from_records`` makes one from the records of a known complex).  ``contacts`` names the
        planes (``pose_fingerprints.planes``: ``None`` = every contact but bare proximity), ``interacting_entities`` the kinds
        of entities whose records take part.  Every chunk of ``chunk`` global poses (default: all at once; a ligand's poses may
        be cut between two) is one ``Context.library_summary``, ``library_fingerprints`` and ``library_fingerprints_best``;
        the chunks are merged (``pose_fingerprints.merge``, ``library_fingerprints.merge_best``).  Returns the result
        ``pose_fingerprints`` describes with the reference rows moved to ``reference_count`` / ``reference_cross``, ``count`` [T],
        ``cross`` [T, Q], and with ``best`` (the table ``library_fingerprints`` describes) and ``ligand_pose_off``; also kept in
        ``self.library_fingerprints``.  The results of ``run_arpeggio`` and ``run_poses`` stay as they are.

        ``classes`` names ring / amide classes as further planes (``pose_fingerprints.planes``: names of ``CLASS_PLANE_NAMES``,
        a table, or 'all'; ``contacts=[]`` gives them alone): pi-stacking, cation-pi, donor-pi, halogen-pi, Met-sulphur-pi and
        amide stacking of every pose, residue level only (``level='atom'`` raises ``ValueError``).  Every chunk is then also one
        ``Context.library_planes_summary`` on the same poses (the ligand packs need ``ring_atoms`` and ``amide_atoms``), and the
        reference masks may carry the class planes (``library_fingerprints.reference_from_plane_records``)."""
        from .. import _capi, contact_filter, ligand_library as _ll, library_fingerprints as _lfp
        if level not in _lfp.LEVELS:
            raise ValueError(f"run_library_fingerprints: level must be 'residue' or 'atom', not {level!r}")
        with_classes = len((classes,) if isinstance(classes, str) else tuple(classes)) > 0
        if with_classes and level != 'residue':
            raise ValueError("run_library_fingerprints: ring / amide classes need level='residue' (their nodes are residues)")
        mask = _lfp.planes(contacts, classes)
        ctype_mask = contact_filter.masks(None, interacting_entities)[1]
        lib = library if isinstance(library, dict) else _ll.pack(list(library))
        n_nodes = self.pc.n_residues if level == 'residue' else self.pc.n_atoms
        r = _lfp.validate(refs, n_nodes, with_classes) if isinstance(refs, dict) else _lfp.references(refs, n_nodes, with_classes)
        if _lfp.n_references(r) < 1:
            raise ValueError('run_library_fingerprints: 1 ... MAX_REFS references')
        off = np.ascontiguousarray(pose_off, np.int64)
        if off.shape != (_ll.n_ligands(lib) + 1,) or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] < 1:
            raise ValueError('run_library_fingerprints: pose_off must be [L + 1], start at 0, not decrease and hold a pose')
        if self._ctx is None:
            self.initialize()
        ctx = self._ctx
        ctx.set_ligand_library(lib)
        if with_classes:
            ctx.set_ligand_library_planes(lib)
        h = np.zeros(0) if h_xyz is None else h_xyz
        parts, bests = [], []
        for off_c, a, _, xc, hc in _ll.chunk_poses(lib, off, xyz, h, chunk if chunk else _capi.POSES_MAX_POSES):
            ctx.library_summary(off_c, xc, hc, interacting_cutoff, vdw_comp, False)
            if with_classes:
                ctx.library_planes_summary(off_c, xc)
            parts.append(ctx.library_fingerprints(r, mask, ctype_mask, by_residue=level == 'residue'))
            bests.append((ctx.library_fingerprints_best(), a))
        out = _lfp.strip_references(parts[0] if len(parts) == 1 else _lfp.merge(parts))
        out['best'] = bests[0][0] if len(bests) == 1 else _lfp.merge_best(bests)
        out['ligand_pose_off'] = off
        self.library_fingerprints = out
        self.library_fingerprints_ligands = lib.get('ligands')
        return out

    def write_library_fingerprints(self, wd):
        """'<id>.libraryfp': the best pose per ligand and reference of the last ``run_library_fingerprints`` as CSV
        (``library_fingerprints.write_csv``)."""
        from .. import library_fingerprints as _lfp
        fp = getattr(self, 'library_fingerprints', None)
        if fp is None:
            raise AttributeError('no library fingerprints yet: call run_library_fingerprints() first')
        return _lfp.write_library_fingerprints(wd, self.id, fp['best'], fp['reference_count'], fp['ligand_pose_off'],
                                               getattr(self, 'library_fingerprints_ligands', None))

    def run_library_shortlist(self, library, pose_off, xyz, h_xyz, k, by='summary', unit='ligands', weights=None, refs=None, min_score=None,
                              planes=False, chunk=None, contacts=None, interacting_entities=None, level='residue', interacting_cutoff=5.0,
                              vdw_comp=0.1):
        """Extension beside the mirror: the best ``k`` ligands of a library (``unit='ligands'``: each by its best pose) or its best
        ``k`` global poses (``unit='poses'``), ranked ON THE DEVICE, with the chosen poses' records — no other pose's record is
        copied (``arpeggio_amd.library_shortlist``).  ``library``, ``pose_off``, ``xyz`` and ``h_xyz`` as
        ``run_library_fingerprints`` takes them.  ``by='summary'``: the score is ``weights`` (``library_shortlist.weights``;
        default: one per record) times the summary slots; ``by='tanimoto'``: the Tanimoto similarity of the pose's fingerprint
        (``contacts`` as ``library_fingerprints.planes`` reads it, at ``level``) to the references ``refs``
        (``library_fingerprints.references``), the best over them, in 32 fractional bits.  Higher is better, a tie goes to the
        lower global pose; ``min_score`` drops entries below it.  ``contacts`` / ``interacting_entities`` also name the records
        that are fetched (``contact_filter.masks``; ``None`` = all).  ``planes=True``: the ring and amide tables of the chosen
        poses as well, and the planes half of ``weights`` (the ligand packs need ``ring_atoms`` and ``amide_atoms``).  Every chunk
        of ``chunk`` global poses (default: all at once; a ligand's poses may be cut between two) is one
        ``Context.library_summary`` (``library_planes_summary``, ``library_fingerprints``) and
        ``Context.library_shortlist(k)`` — no full fetch; the chunks' shortlists are shifted to the caller's global poses and
        merged on the host (``library_shortlist.merge``).  Returns the shortlist ``arpeggio_amd.library_shortlist`` describes
        (also kept in ``self.library_shortlist``, the ligands in ``self.library_shortlist_ligands``)."""
        from .. import _capi, contact_filter, ligand_library as _ll, library_fingerprints as _lfp, library_shortlist as _lsl
        if by not in ('summary', 'tanimoto'):
            raise ValueError(f"run_library_shortlist: by must be 'summary' or 'tanimoto', not {by!r}")
        if unit not in _lsl.UNITS:
            raise ValueError(f'run_library_shortlist: unit must be one of {_lsl.UNITS}')
        if int(k) < 1:
            raise ValueError('run_library_shortlist: k must be at least 1')
        sift_mask = 0 if contacts is None else contact_filter.masks(contacts, None)[0]
        ctype_mask = contact_filter.masks(None, interacting_entities)[1]
        lib = library if isinstance(library, dict) else _ll.pack(list(library))
        off = np.ascontiguousarray(pose_off, np.int64)
        if off.shape != (_ll.n_ligands(lib) + 1,) or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] < 1:
            raise ValueError('run_library_shortlist: pose_off must be [L + 1], start at 0, not decrease and hold a pose')
        if by == 'tanimoto':
            if level not in _lfp.LEVELS:
                raise ValueError(f"run_library_shortlist: level must be 'residue' or 'atom', not {level!r}")
            n_nodes = self.pc.n_residues if level == 'residue' else self.pc.n_atoms
            r = _lfp.validate(refs, n_nodes) if isinstance(refs, dict) else _lfp.references(refs or [], n_nodes)
            if _lfp.n_references(r) < 1:
                raise ValueError('run_library_shortlist: 1 ... MAX_REFS references')
            fp_planes = _lfp.planes(contacts)
        elif weights is None:
            weights = _lsl.weights(atom_atom={'records': 1})
        if self._ctx is None:
            self.initialize()
        ctx = self._ctx
        ctx.set_ligand_library(lib)
        if planes:
            ctx.set_ligand_library_planes(lib)
        tables = _lsl.TABLES if planes else ('atom_atom',)
        h = np.zeros(0) if h_xyz is None else h_xyz
        parts = []
        for off_c, a, _, xc, hc in _ll.chunk_poses(lib, off, xyz, h, chunk if chunk else _capi.POSES_MAX_POSES):
            ctx.library_summary(off_c, xc, hc, interacting_cutoff, vdw_comp, False)
            if planes:
                ctx.library_planes_summary(off_c, xc)
            if by == 'tanimoto':
                ctx.library_fingerprints(r, fp_planes, ctype_mask, by_residue=level == 'residue')
                part = ctx.library_shortlist('tanimoto', unit=unit, ref=-1, k=int(k), min_score=min_score, tables=tables, sift_mask=sift_mask,
                                             ctype_mask=ctype_mask)
            else:
                part = ctx.library_shortlist('summary', unit=unit, weights=weights, k=int(k), min_score=min_score, tables=tables,
                                             sift_mask=sift_mask, ctype_mask=ctype_mask)
            parts.append(_lsl.shift(part, a))
        out = _lsl.merge(parts, int(k), unit)
        out.update(by=by, unit=unit)
        self.library_shortlist = out
        self.library_shortlist_ligands = lib.get('ligands')
        return out

    def write_library_shortlist(self, wd):
        """'<id>.libraryshortlist': the atom-atom records of the last ``run_library_shortlist`` as CSV
        (``library_shortlist.write_csv``)."""
        from .. import library_shortlist as _lsl
        if getattr(self, 'library_shortlist', None) is None:
            raise AttributeError('no library shortlist yet: call run_library_shortlist() first')
        if getattr(self, 'library_shortlist_ligands', None) is None:
            raise AttributeError('the library of the last run_library_shortlist() carried no ligand packs (labels)')
        return _lsl.write_library_shortlist(wd, self.id, self.library_shortlist, self.pc, self.library_shortlist_ligands, self.component_types)

    def run_library_clusters(self, library, pose_off, xyz, h_xyz, k, threshold=0.5, by='summary', unit='ligands', weights=None, refs=None,
                             max_clusters=256, records=False, contacts=None, interacting_entities=None, level='residue',
                             interacting_cutoff=5.0, vdw_comp=0.1):
        """Extension beside the mirror: the DIVERSE hits of a library — its best ``k`` ligands (``unit='ligands'``) or global poses
        ranked as ``run_library_shortlist`` ranks them, then clustered in rank order ON THE DEVICE by the Tanimoto similarity of
        their library fingerprints (``arpeggio_amd.library_clusters``): one representative per interaction pattern, how many
        entries stand behind it, and their ligands.  ``library``, ``pose_off``, ``xyz``, ``h_xyz``, ``by``, ``unit``, ``weights``
        and ``refs`` as ``run_library_shortlist`` takes them (``refs`` may be empty for ``by='summary'``); ``contacts`` / ``level``
        name the fingerprint's planes and nodes.  Two poses are similar when their similarity is at least ``threshold``
        (a float in [0, 1]); a pose joins the FIRST similar leader in rank order.  One launch each of
        ``Context.library_summary``, ``library_fingerprints``, ``library_shortlist`` and ``library_clusters(source='shortlist')``:
        no bit crosses to the host.  ``records=True``: also ``representatives``, a ``library_shortlist('list')`` over the
        leaders — only the representatives' records are copied.  There is no ``chunk``: a clustering does not decompose over
        launches, and a library of more than ``_capi.POSES_MAX_POSES`` global poses is refused.  Returns the clusters
        ``arpeggio_amd.library_clusters`` describes (also kept in ``self.library_clusters``)."""
        from .. import _capi, contact_filter, ligand_library as _ll, library_clusters as _lcl, library_fingerprints as _lfp, library_shortlist as _lsl
        if by not in ('summary', 'tanimoto'):
            raise ValueError(f"run_library_clusters: by must be 'summary' or 'tanimoto', not {by!r}")
        if unit not in _lsl.UNITS:
            raise ValueError(f'run_library_clusters: unit must be one of {_lsl.UNITS}')
        if int(k) < 1:
            raise ValueError('run_library_clusters: k must be at least 1')
        if level not in _lfp.LEVELS:
            raise ValueError(f"run_library_clusters: level must be 'residue' or 'atom', not {level!r}")
        thr = _lcl.threshold_q32(threshold)
        lib = library if isinstance(library, dict) else _ll.pack(list(library))
        off = np.ascontiguousarray(pose_off, np.int64)
        if off.shape != (_ll.n_ligands(lib) + 1,) or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] < 1:
            raise ValueError('run_library_clusters: pose_off must be [L + 1], start at 0, not decrease and hold a pose')
        if len(_ll.chunk_plan(off, _capi.POSES_MAX_POSES)) != 1:
            raise ValueError(f'run_library_clusters: {int(off[-1])} global poses are more than one launch takes ({_capi.POSES_MAX_POSES}); '
                             'a clustering does not decompose over launches (shortlist the library in chunks first)')
        n_nodes = self.pc.n_residues if level == 'residue' else self.pc.n_atoms
        r = _lfp.validate(refs, n_nodes) if isinstance(refs, dict) else _lfp.references(refs or [], n_nodes)
        if by == 'tanimoto' and _lfp.n_references(r) < 1:
            raise ValueError('run_library_clusters: 1 ... MAX_REFS references (by tanimoto)')
        if by == 'summary' and weights is None:
            weights = _lsl.weights(atom_atom={'records': 1})
        ctype_mask = contact_filter.masks(None, interacting_entities)[1]
        if self._ctx is None:
            self.initialize()
        ctx = self._ctx
        ctx.set_ligand_library(lib)
        ctx.library_summary(off, xyz, np.zeros(0) if h_xyz is None else h_xyz, interacting_cutoff, vdw_comp, False)
        ctx.library_fingerprints(r, _lfp.planes(contacts), ctype_mask, by_residue=level == 'residue')
        if by == 'tanimoto':
            ctx.library_shortlist('tanimoto', unit=unit, ref=-1, k=int(k), tables=('atom_atom',), ctype_mask=ctype_mask)
        else:
            ctx.library_shortlist('summary', unit=unit, weights=weights, k=int(k), tables=('atom_atom',), ctype_mask=ctype_mask)
        out = ctx.library_clusters(thr, source='shortlist', max_clusters=max_clusters)
        out.update(by=by, unit=unit)
        if records:
            out['representatives'] = ctx.library_shortlist('list', pose_ids=out['leader'], tables=('atom_atom',), ctype_mask=ctype_mask)
        self.library_clusters = out
        return out

    def write_library_clusters(self, wd):
        """'<id>.libraryclusters': the clusters of the last ``run_library_clusters`` as CSV (``library_clusters.write_csv``)."""
        from .. import library_clusters as _lcl
        if getattr(self, 'library_clusters', None) is None:
            raise AttributeError('no library clusters yet: call run_library_clusters() first')
        return _lcl.write_library_clusters(wd, self.id, self.library_clusters)

    def write_pose_planes(self, wd):
        """'<id>.poseplanes': the ring / amide tables of the last ``run_poses(..., planes=True)`` as CSV (``poses.write_planes_csv``)."""
        from .. import poses as _poses
        if getattr(self, 'pose_planes', None) is None:
            raise AttributeError('no pose planes yet: call run_poses(..., planes=True) first')
        return _poses.write_pose_planes(wd, self.id, self.pose_planes, self.pc, self.component_types)

    def run_pose_fingerprints(self, user_selections, xyz, h_xyz, interacting_cutoff, vdw_comp, include_sequence_adjacent,
                              refs_xyz=None, refs_h_xyz=None, contacts=None, interacting_entities=None, level='residue', chunk=None,
                              all_pairs=False, classes=()):
        """Extension beside the mirror: the interaction fingerprints of many poses of a ligand scored against reference poses ON
        THE DEVICE — no record is copied.  Selection, ``xyz``, ``h_xyz`` and the three parameters are those of ``run_poses``.
        ``refs_xyz`` float32 [Q, S, 3] / ``refs_h_xyz`` float64 [Q, SH, 3] are the reference poses (at most
        ``pose_fingerprints.MAX_REFS``); the default is the resident coordinates of the movable set, Q = 1.  A feature is
        (receptor residue or, ``level='atom'``, receptor atom; contact): ``contacts`` names the contacts
        (``pose_fingerprints.planes``: ``None`` = every contact but bare proximity), ``interacting_entities`` the kinds of
        entities whose records take part (``contact_filter.masks``; ``None`` = all).  Every chunk of ``chunk`` poses (default:
        all at once) is launched as references ++ chunk (``Context.poses_summary``, then ``Context.poses_fingerprints``) and the
        chunks are merged (``pose_fingerprints.merge``).  Returns the result ``arpeggio_amd.pose_fingerprints`` describes, with the
        reference rows moved to ``reference_count`` / ``reference_cross`` (also kept in ``self.pose_fingerprints``): ``count`` [P],
        ``cross`` [P, Q], ``occupancy`` over the P poses.  ``all_pairs=True`` adds ``inter`` uint32 [P, P] (one chunk of at most
        ``similarity.MAX_MODELS`` - Q poses).  ``classes`` adds the ring and amide classes as planes
        (``pose_fingerprints.planes``: names of ``CLASS_PLANE_NAMES``, a table's name or 'all'; residue level only; the pack
        needs ``ring_atoms`` and ``amide_atoms``): every chunk is then also launched as ``Context.poses_planes_summary`` on
        the same references ++ chunk coordinates, and both resident results are reduced into one matrix."""
        from .. import _capi, contact_filter, poses as _poses, pose_fingerprints as _fp
        if level not in _fp.LEVELS:
            raise ValueError(f"run_pose_fingerprints: level must be 'residue' or 'atom', not {level!r}")
        mask = _fp.planes(contacts, classes)
        with_classes = (mask >> _fp.N_PLANES) != 0
        if with_classes and level != 'residue':
            raise ValueError("run_pose_fingerprints: the ring / amide class planes exist at level='residue' only")
        ctype_mask = contact_filter.masks(None, interacting_entities)[1]
        if self._ctx is None:
            self.initialize()
        pc, ctx = self.pc, self._ctx
        if isinstance(user_selections, np.ndarray):
            idx = np.unique(user_selections.astype(np.int64))
        else:
            idx = utils.selection_parser(user_selections, pc) if user_selections else np.zeros(0, np.int64)
        if idx.size == 0:
            raise AttributeError('Selection must not be empty.')
        sel = np.zeros(pc.n_atoms, np.uint8)
        sel[idx] = 1
        atoms, rows = _poses.movable(pc, idx)
        x = np.ascontiguousarray(xyz, np.float32)
        h = np.zeros((len(x), 0, 3)) if h_xyz is None else np.ascontiguousarray(h_xyz, np.float64)
        if refs_xyz is None:
            rx = np.asarray(pc.xyz, np.float32)[atoms][None]
            rh = np.asarray(pc.h_xyz, np.float64).reshape(-1, 3)[rows][None]
        else:
            rx = np.ascontiguousarray(refs_xyz, np.float32)
            rh = np.zeros((len(rx), 0, 3)) if refs_h_xyz is None else np.ascontiguousarray(refs_h_xyz, np.float64)
        Q = len(rx)
        if not 1 <= Q <= _fp.MAX_REFS:
            raise ValueError(f'run_pose_fingerprints: 1 ... {_fp.MAX_REFS} reference poses')
        if len(x) < 1:
            raise ValueError('run_pose_fingerprints: no pose given')
        if x.shape[1:] != rx.shape[1:] or h.shape[1:] != rh.shape[1:]:
            raise ValueError('run_pose_fingerprints: the references and the poses must have the same atoms and hydrogen rows')
        step = int(chunk) if chunk else min(len(x), _capi.POSES_MAX_POSES - Q)
        if step < 1:
            raise ValueError('run_pose_fingerprints: chunk must be at least 1')
        if all_pairs and step < len(x):
            raise ValueError('run_pose_fingerprints: all_pairs needs all poses in one chunk')
        ctx.set_selection(sel)
        if with_classes:
            ctx.set_plane_atoms(pc)
        parts = []
        for a in range(0, len(x), step):
            both = np.concatenate([rx, x[a:a + step]])
            ctx.poses_summary(both, np.concatenate([rh, h[a:a + step]]), interacting_cutoff, vdw_comp, include_sequence_adjacent)
            if with_classes:
                ctx.poses_planes_summary(both)
            parts.append(ctx.poses_fingerprints(mask, ctype_mask, by_residue=level == 'residue', n_refs=Q, all_pairs=all_pairs))
        out = _fp.strip_references(parts[0] if len(parts) == 1 else _fp.merge(parts))
        if all_pairs:
            out['inter'] = np.ascontiguousarray(parts[0]['inter'][Q:, Q:])
        self.pose_fingerprints = out
        return out

    def write_pose_fingerprints(self, wd):
        """'<id>.posefp': the result of the last ``run_pose_fingerprints`` as CSV (``pose_fingerprints.write_csv``)."""
        from .. import pose_fingerprints as _fp
        if getattr(self, 'pose_fingerprints', None) is None:
            raise AttributeError('no pose fingerprints yet: call run_pose_fingerprints() first')
        return _fp.write_pose_fingerprints(wd, self.id, self.pose_fingerprints, self.pc, self.component_types)

    def run_pose_shortlist(self, user_selections, xyz, h_xyz, interacting_cutoff, vdw_comp, include_sequence_adjacent, k, by='summary',
                           weights=None, refs_xyz=None, refs_h_xyz=None, contacts=None, interacting_entities=None, min_score=None,
                           planes=False, chunk=None):
        """Extension beside the mirror: the best ``k`` of many poses of a ligand, ranked ON THE DEVICE, with their records — no
        other pose's record is copied.  Selection, ``xyz``, ``h_xyz`` and the three parameters are those of ``run_poses``.
        ``by='summary'``: the score is ``weights`` (``pose_shortlist.weights``; default: one per record) times the summary
        slots; ``by='tanimoto'``: the Tanimoto similarity of the pose's fingerprint (``contacts`` as
        ``pose_fingerprints.planes`` reads it, residue level) to the reference poses ``refs_xyz`` / ``refs_h_xyz`` (default: the
        resident coordinates), the best over the references, in 32 fractional bits.  Higher is better, a tie goes to the lower
        pose id; ``min_score`` drops poses below it.  ``contacts`` / ``interacting_entities`` also name the records that are
        fetched (``contact_filter.masks``; ``None`` = all).  ``planes=True``: the ring and amide tables of the chosen poses as
        well, and the planes half of ``weights`` (the pack needs ``ring_atoms`` and ``amide_atoms``).  Every chunk of ``chunk``
        poses (default: all at once) is launched as ``Context.poses_summary`` (``poses_planes_summary``,
        ``poses_fingerprints`` with the references in front) and ``Context.poses_shortlist(k)``; the chunks' shortlists are
        merged on the host (``pose_shortlist.merge``).  Returns the shortlist ``arpeggio_amd.pose_shortlist`` describes, ``pose``
        in the caller's numbering (also kept in ``self.pose_shortlist``)."""
        from .. import _capi, contact_filter, poses as _poses, pose_fingerprints as _fp, pose_shortlist as _sl
        if by not in ('summary', 'tanimoto'):
            raise ValueError(f"run_pose_shortlist: by must be 'summary' or 'tanimoto', not {by!r}")
        if int(k) < 1:
            raise ValueError('run_pose_shortlist: k must be at least 1')
        sift_mask = 0 if contacts is None else contact_filter.masks(contacts, None)[0]
        ctype_mask = contact_filter.masks(None, interacting_entities)[1]
        if self._ctx is None:
            self.initialize()
        pc, ctx = self.pc, self._ctx
        if isinstance(user_selections, np.ndarray):
            idx = np.unique(user_selections.astype(np.int64))
        else:
            idx = utils.selection_parser(user_selections, pc) if user_selections else np.zeros(0, np.int64)
        if idx.size == 0:
            raise AttributeError('Selection must not be empty.')
        sel = np.zeros(pc.n_atoms, np.uint8)
        sel[idx] = 1
        atoms, rows = _poses.movable(pc, idx)
        x = np.ascontiguousarray(xyz, np.float32)
        h = np.zeros((len(x), 0, 3)) if h_xyz is None else np.ascontiguousarray(h_xyz, np.float64)
        if len(x) < 1:
            raise ValueError('run_pose_shortlist: no pose given')
        Q = 0
        if by == 'tanimoto':
            if refs_xyz is None:
                rx = np.asarray(pc.xyz, np.float32)[atoms][None]
                rh = np.asarray(pc.h_xyz, np.float64).reshape(-1, 3)[rows][None]
            else:
                rx = np.ascontiguousarray(refs_xyz, np.float32)
                rh = np.zeros((len(rx), 0, 3)) if refs_h_xyz is None else np.ascontiguousarray(refs_h_xyz, np.float64)
            Q = len(rx)
            if not 1 <= Q <= _fp.MAX_REFS:
                raise ValueError(f'run_pose_shortlist: 1 ... {_fp.MAX_REFS} reference poses')
            if x.shape[1:] != rx.shape[1:] or h.shape[1:] != rh.shape[1:]:
                raise ValueError('run_pose_shortlist: the references and the poses must have the same atoms and hydrogen rows')
            fp_planes = _fp.planes(contacts)
        elif weights is None:
            weights = _sl.weights(atom_atom={'records': 1})
        step = int(chunk) if chunk else min(len(x), _capi.POSES_MAX_POSES - Q)
        if step < 1:
            raise ValueError('run_pose_shortlist: chunk must be at least 1')
        tables = _sl.TABLES if planes else ('atom_atom',)
        ctx.set_selection(sel)
        if planes:
            ctx.set_plane_atoms(pc)
        parts = []
        for a in range(0, len(x), step):
            cx, ch = x[a:a + step], h[a:a + step]
            if Q:
                cx, ch = np.concatenate([rx, cx]), np.concatenate([rh, ch])
            ctx.poses_summary(cx, ch, interacting_cutoff, vdw_comp, include_sequence_adjacent)
            if planes:
                ctx.poses_planes_summary(cx)
            if by == 'tanimoto':
                ctx.poses_fingerprints(fp_planes, ctype_mask, by_residue=True, n_refs=Q)
                part = ctx.poses_shortlist('tanimoto', ref=-1, skip=Q, k=int(k), min_score=min_score, tables=tables, sift_mask=sift_mask,
                                           ctype_mask=ctype_mask)
            else:
                part = ctx.poses_shortlist('summary', weights=weights, k=int(k), min_score=min_score, tables=tables, sift_mask=sift_mask,
                                           ctype_mask=ctype_mask)
            parts.append(_sl.shift(part, a - Q))
        out = _sl.merge(parts, int(k))
        out.update(by=by, n_refs=Q)
        self.pose_shortlist = out
        return out

    def write_pose_shortlist(self, wd):
        """'<id>.shortlist': the atom-atom records of the last ``run_pose_shortlist`` as CSV (``pose_shortlist.write_csv``)."""
        from .. import pose_shortlist as _sl
        if getattr(self, 'pose_shortlist', None) is None:
            raise AttributeError('no pose shortlist yet: call run_pose_shortlist() first')
        return _sl.write_pose_shortlist(wd, self.id, self.pose_shortlist, self.pc, self.component_types)

    def run_pose_clusters(self, user_selections, xyz, h_xyz, interacting_cutoff, vdw_comp, include_sequence_adjacent, threshold=0.5,
                          by='summary', weights=None, refs_xyz=None, refs_h_xyz=None, contacts=None, interacting_entities=None, level='residue',
                          classes=(), max_clusters=256, records=False):
        """Extension beside the mirror: many poses of a ligand grouped into binding modes ON THE DEVICE — leader clustering in rank
        order by the Tanimoto similarity of their interaction fingerprints; no record and no fingerprint is copied.  Selection,
        ``xyz``, ``h_xyz`` and the three parameters are those of ``run_poses``; ``refs_xyz`` / ``refs_h_xyz`` (default: the
        resident coordinates), ``contacts``, ``interacting_entities``, ``level`` and ``classes`` those of
        ``run_pose_fingerprints``.  The poses are walked from best to worst: ``by='summary'`` ranks by ``weights``
        (``pose_shortlist.weights``; default: one per record) times the summary slots, ``by='tanimoto'`` by the best similarity
        to a reference pose, ``by='input'`` keeps the order given; a tie goes to the lower pose id.  A pose whose similarity to
        an earlier leader is at least ``threshold`` (a float in [0, 1], ``pose_clusters.threshold_q32``) joins the first such
        leader, otherwise it leads a new cluster — at most ``max_clusters``, the poses after that stay unassigned.  One launch
        of references ++ poses (``Context.poses_summary``, ``poses_planes_summary`` with ``classes``,
        ``poses_fingerprints``), the rank order on the host from what those calls copied anyway, ``Context.poses_clusters``.
        There is no ``chunk``: a clustering does not decompose over launches (a pose's leader may sit in any other chunk), so
        references and poses together are at most ``_capi.POSES_MAX_POSES``.  Returns the dict ``arpeggio_amd.pose_clusters``
        describes, pose ids in the caller's numbering, with ``by`` and ``n_refs`` (also kept in ``self.pose_clusters``);
        ``records=True`` adds ``'records'``: the atom-atom records of the leaders as a shortlist
        (``Context.poses_shortlist('list', ...)``), ``pose`` in the caller's numbering."""
        from .. import _capi, contact_filter, poses as _poses, pose_clusters as _cl, pose_fingerprints as _fp, pose_shortlist as _sl
        if by not in ('summary', 'tanimoto', 'input'):
            raise ValueError(f"run_pose_clusters: by must be 'summary', 'tanimoto' or 'input', not {by!r}")
        if level not in _fp.LEVELS:
            raise ValueError(f"run_pose_clusters: level must be 'residue' or 'atom', not {level!r}")
        thr = _cl.threshold_q32(threshold)
        if not 1 <= int(max_clusters) <= _cl.MAX_CLUSTERS:
            raise ValueError(f'run_pose_clusters: max_clusters must be 1 ... {_cl.MAX_CLUSTERS}')
        mask = _fp.planes(contacts, classes)
        with_classes = (mask >> _fp.N_PLANES) != 0
        if with_classes and level != 'residue':
            raise ValueError("run_pose_clusters: the ring / amide class planes exist at level='residue' only")
        ctype_mask = contact_filter.masks(None, interacting_entities)[1]
        if self._ctx is None:
            self.initialize()
        pc, ctx = self.pc, self._ctx
        if isinstance(user_selections, np.ndarray):
            idx = np.unique(user_selections.astype(np.int64))
        else:
            idx = utils.selection_parser(user_selections, pc) if user_selections else np.zeros(0, np.int64)
        if idx.size == 0:
            raise AttributeError('Selection must not be empty.')
        sel = np.zeros(pc.n_atoms, np.uint8)
        sel[idx] = 1
        atoms, rows = _poses.movable(pc, idx)
        x = np.ascontiguousarray(xyz, np.float32)
        h = np.zeros((len(x), 0, 3)) if h_xyz is None else np.ascontiguousarray(h_xyz, np.float64)
        if refs_xyz is None:
            rx = np.asarray(pc.xyz, np.float32)[atoms][None]
            rh = np.asarray(pc.h_xyz, np.float64).reshape(-1, 3)[rows][None]
        else:
            rx = np.ascontiguousarray(refs_xyz, np.float32)
            rh = np.zeros((len(rx), 0, 3)) if refs_h_xyz is None else np.ascontiguousarray(refs_h_xyz, np.float64)
        Q = len(rx)
        if not 1 <= Q <= _fp.MAX_REFS:
            raise ValueError(f'run_pose_clusters: 1 ... {_fp.MAX_REFS} reference poses')
        if len(x) < 1:
            raise ValueError('run_pose_clusters: no pose given')
        if Q + len(x) > _capi.POSES_MAX_POSES:
            raise ValueError('run_pose_clusters: references and poses together exceed one launch (a clustering does not decompose over launches)')
        if x.shape[1:] != rx.shape[1:] or h.shape[1:] != rh.shape[1:]:
            raise ValueError('run_pose_clusters: the references and the poses must have the same atoms and hydrogen rows')
        if by == 'summary' and weights is None:
            weights = _sl.weights(atom_atom={'records': 1})
        ctx.set_selection(sel)
        if with_classes:
            ctx.set_plane_atoms(pc)
        both = np.concatenate([rx, x])
        summary = ctx.poses_summary(both, np.concatenate([rh, h]), interacting_cutoff, vdw_comp, include_sequence_adjacent)
        planes_summary = ctx.poses_planes_summary(both) if with_classes else None
        f = ctx.poses_fingerprints(mask, ctype_mask, by_residue=level == 'residue', n_refs=Q)
        if by == 'summary':
            if planes_summary is None and np.asarray(weights).reshape(-1)[16:].any():
                raise ValueError('run_pose_clusters: a weight on a planes slot needs classes (the ring and amide contacts)')
            rank = _sl.order(_sl.scores('summary', summary=summary, planes_summary=planes_summary, w=weights), Q)
        elif by == 'tanimoto':
            rank = _sl.order(_sl.tanimoto_q32(f['count'], f['cross'], Q, -1), Q)
        else:
            rank = np.arange(Q, Q + len(x), dtype=np.int64)
        out = _cl.shift(ctx.poses_clusters(thr, order=rank, max_clusters=int(max_clusters)), -Q)
        out.update(by=by, n_refs=Q, level=level)
        if records:
            out['records'] = _sl.shift(ctx.poses_shortlist('list', pose_ids=np.asarray(out['leader']) + Q), -Q)
        self.pose_clusters = out
        return out

    def write_pose_clusters(self, wd):
        """'<id>.poseclusters': the clusters of the last ``run_pose_clusters`` as CSV, one row per position (``pose_clusters.write_csv``)."""
        from .. import pose_clusters as _cl
        if getattr(self, 'pose_clusters', None) is None:
            raise AttributeError('no pose clusters yet: call run_pose_clusters() first')
        return _cl.write_pose_clusters(wd, self.id, self.pose_clusters)

    # ---- the legacy CSV tables (I:135-170, 349-366, 405-466) ----
    def write_atom_types(self, wd):
        """I:135-149: '<id>_atomtypes.csv'."""
        export.write_atom_types(wd, self.id, self.pc, self.component_types)
        logging.debug('Typed atoms.')

    def write_contacts(self, selection, wd):
        """I:151-170: '<id>_contacts.csv' (+ '<id>_bs_contacts.csv' when ``selection`` is not empty)."""
        self._need_results()
        export.write_contacts(wd, self.id, self.pc, self._bags['atom_atom'], self.component_types, len(selection) > 0)

    def write_atom_sifts(self, wd):
        """I:349-366, 576-606: '<id>_sifts.csv' (atom, 15 flags) and '<id>_specific_sifts.csv' (atom, inter / intra /
        water flags, 45 columns) for the atoms of selection_plus, in packed atom order (the reference iterates a set).
        The header row is the reference's (17 names whatever the row width)."""
        import csv
        a = self.atom_sifts()
        lab = export.Labels(self.pc, self.component_types)
        header = ['atom'] + list(config.SIFT_NAMES) + ['interacting_entities']
        rows_all, rows_spec = [], []
        for i in self.selection_plus.tolist():
            label = lab.atom_macro(i)
            rows_all.append([label] + a['sift'][i].tolist())
            rows_spec.append([label] + a['sift_inter_only'][i].tolist() + a['sift_intra_only'][i].tolist()
                             + a['sift_water_only'][i].tolist())
        for name, rows in ((self.id + '_sifts.csv', rows_all), (self.id + '_specific_sifts.csv', rows_spec)):
            with open(os.path.join(wd, name), 'w') as f:
                w = csv.writer(f, delimiter=',', quotechar='"', quoting=csv.QUOTE_MINIMAL)
                w.writerow(header)
                w.writerows(rows)

    def write_residue_sifts(self, wd):
        """I:435-466: '<id>_residue_sifts.csv', one row of 426 columns per residue of selection_plus."""
        export.write_residue_sifts(wd, self.id, self.pc, self.component_types, self.selection_plus_residues, self.residue_sifts())

    def write_polar_matching(self, wd):
        """I:405-433: '<id>_polarmatch.csv' and '<id>_specific_polarmatch.csv' for the atoms of selection_plus."""
        export.write_polar_matching(wd, self.id, self.pc, self.component_types, self.selection_plus, self.atom_sifts()['counts'])

    def write_binding_site_sifts(self, wd):
        """I:368-403 cannot complete in the reference itself: its row expression indexes a list with a list (I:401-402,
        a missing ``+``) and ``utils.int3`` needs ``collections.Iterable`` (U:388, gone since Python 3.10), so there is no
        output to reproduce.  ``potential_fsift()`` gives the per-atom potential feature SIFt it would match against."""
        raise NotImplementedError('write_binding_site_sifts raises TypeError in the reference (interactions.py:401-402); '
                                  'see potential_fsift() / atom_sifts() for its inputs')

    def minimize_hydrogens(self, minimisation_forcefield='MMFF94', minimisation_method='ConjugateGradients', minimisation_steps=50):
        """I:214-269 is an OpenBabel force-field run over the hydrogens before ``initialize()`` — SURVEY row 9, outside the
        path this package replaces.  Run it with the reference (or any tool) and hand over the hydrogenated file."""
        raise NotImplementedError('minimize_hydrogens is OpenBabel force-field code (interactions.py:214-269), outside the '
                                  'run_arpeggio path: minimise with OpenBabel first and pass the resulting mmCIF file')

    def write_hydrogenated(self, wd, input_structure):
        """I:271-286 writes OpenBabel's molecule after hydrogen addition; this package adds no hydrogens (see ``read_mmcif``)."""
        raise NotImplementedError('write_hydrogenated writes OpenBabel\'s hydrogenated molecule (interactions.py:271-286); '
                                  'this package does not add hydrogens')

    def potential_fsift(self):
        """``atom.potential_fsift`` (I:1795-1852) as uint8 [n_atoms, 10]."""
        m = export.potential_fsift(self.pc)
        return ((m[:, None] >> np.arange(10, dtype=np.uint16)[None, :]) & 1).astype(np.uint8)

    def get_contacts(self, share_atoms=False):
        """I:172-212: the JSON-able list of contact records, bags in the reference's order (atom-atom, plane-plane,
        atom-plane, group-group, group-plane), canonical order inside a bag ([] before run_arpeggio, like I:84-88).
        ``share_atoms=True`` (not in the reference): records of the same atom share their inner dictionary — same JSON,
        less than half the time on a whole-structure run; see ``export.contacts_json``."""
        return export.contacts_json(self.pc, self._bags, self.component_types, share_atoms)

    def write_json(self, path, indent=4):
        """The file the reference's CLI writes (scripts/process_protein_cli.py:184-188):
        ``json.dump(self.get_contacts(), fh, indent=4, sort_keys=True)``, byte for byte, without building the records in
        Python (native formatter for the atom-atom bag)."""
        export.write_contacts_json(path, self.pc, self._bags, self.component_types, indent)

    # endregion


def residue_plane_sifts(pc, bags):
    """See InteractionComplex.residue_plane_sifts; `bags` = dict of the four ring/amide result bags (arrays)."""
    nr = pc.n_residues
    inter = config.CONTACT_TYPE_NAMES.index('INTER')
    out = {
        'ring_ring_inter_integer_sift': np.zeros((nr, 9), np.int64),
        'ring_atom_inter_integer_sift': np.zeros((nr, 5), np.int64),
        'atom_ring_inter_integer_sift': np.zeros((nr, 5), np.int64),
        'mc_atom_ring_inter_integer_sift': np.zeros((nr, 5), np.int64),
        'sc_atom_ring_inter_integer_sift': np.zeros((nr, 5), np.int64),
        'amide_amide_inter_integer_sift': np.zeros((nr, 1), np.int64),
        'amide_ring_inter_integer_sift': np.zeros((nr, 1), np.int64),
        'ring_amide_inter_integer_sift': np.zeros((nr, 1), np.int64),
    }
    b = bags.get('plane_plane')
    if b is not None and len(b['bgn']):
        r1, r2 = pc.ring_res[b['bgn']], pc.ring_res[b['end']]
        ok = (b['ctype'] == inter) & (r1 != r2)                     # I:1171
        t1, t2 = b['type1'].astype(np.int64), b['type2'].astype(np.int64)
        # the visit that created the record counts for the bgn ring's residue (I:1173-1176) ...
        m = ok & (t1 < 9)
        np.add.at(out['ring_ring_inter_integer_sift'], (r1[m], t1[m]), 1)
        # ... the reverse visit, when it happened, for the end ring's residue with its own class
        rev = np.where(t2 == config.PP_SAME, t1, t2)
        m = ok & (t2 != config.PP_SKIPPED) & (rev < 9)
        np.add.at(out['ring_ring_inter_integer_sift'], (r2[m], rev[m]), 1)
    b = bags.get('atom_plane')
    if b is not None and len(b['atom']):
        ra, rr = pc.res_id[b['atom']], pc.ring_res[b['ring']]
        ok = (b['ctype'] == inter) & (ra != rr)                     # I:1040
        poly = (pc.res_flags[ra] & config.R_POLYPEPTIDE) != 0       # atom.get_parent() in self.polypeptide_residues
        names = np.asarray(pc.atom_name, dtype=object)[b['atom']]
        mc = np.array([n in config.MAINCHAIN_ATOMS for n in names], bool) if len(names) else np.zeros(0, bool)
        for k in range(5):
            m = ok & (((b['mask'] >> k) & 1) == 1)
            np.add.at(out['ring_atom_inter_integer_sift'], (rr[m], k), 1)
            np.add.at(out['atom_ring_inter_integer_sift'], (ra[m], k), 1)
            np.add.at(out['mc_atom_ring_inter_integer_sift'], (ra[m & poly & mc], k), 1)
            np.add.at(out['sc_atom_ring_inter_integer_sift'], (ra[m & poly & ~mc], k), 1)
    b = bags.get('group_group')
    if b is not None and len(b['bgn']):
        r1, r2 = pc.amide_res[b['bgn']], pc.amide_res[b['end']]
        m = (b['ctype'] == inter) & (r1 != r2)                      # I:1290
        np.add.at(out['amide_amide_inter_integer_sift'], (r1[m], 0), 1)
    b = bags.get('group_plane')
    if b is not None and len(b['amide']):
        ra, rr = pc.amide_res[b['amide']], pc.ring_res[b['ring']]
        m = (b['ctype'] == inter) & (ra != rr)                      # I:1371
        np.add.at(out['amide_ring_inter_integer_sift'], (ra[m], 0), 1)
        np.add.at(out['ring_amide_inter_integer_sift'], (rr[m], 0), 1)
    return out


def pack_from_reference_objects(ic, ob=None):
    """Build a PackedComplex from a *reference* ``arpeggio.core.InteractionComplex`` on which ``initialize()`` has run:
    the mapping of I:54-60, 1494-1529, 1591-1733, 1531-1589, 1923-1991 onto the packed arrays.  ``ob``: the OpenBabel
    module (``from openbabel import openbabel``, imported here when not given; the tests pass the iterator holders of
    tests/golden/make_golden_core.py — neither BioPython nor OpenBabel is in this repository's image)."""
    if ob is None:
        from openbabel import openbabel as ob
    atoms = list(ic.s_atoms)
    index = {a: i for i, a in enumerate(atoms)}
    residues, res_index = [], {}
    for a in atoms:
        r = a.get_parent()
        if id(r) not in res_index:
            res_index[id(r)] = len(residues)
            residues.append(r)
    T = config.ATOM_TYPE_BIT
    n = len(atoms)
    xyz = np.array([a.coord for a in atoms], np.float32)
    flags = np.zeros(n, np.uint16)
    tmask = np.zeros(n, np.uint16)
    for i, a in enumerate(atoms):
        tmask[i] = sum(T[t] for t in a.atom_types)
        f = 0
        f |= config.F_METAL if a.is_metal else 0
        f |= config.F_HALOGEN if a.is_halogen else 0
        f |= config.F_WATER if a.get_full_id()[3][0] == 'W' else 0
        f |= config.F_HYDROGEN if a.element.strip() == 'H' else 0
        f |= config.F_ELEM_C if a.element == 'C' else 0
        f |= config.F_ELEM_S if a.element == 'S' else 0
        f |= config.F_RES_MET if a.get_parent().resname == 'MET' else 0
        flags[i] = f
    res_flags = np.zeros(len(residues), np.uint8)
    res_prev = np.full(len(residues), -1, np.int32)
    res_next = np.full(len(residues), -1, np.int32)
    for k, r in enumerate(residues):
        if getattr(r, 'is_polypeptide', False):
            res_flags[k] |= config.R_POLYPEPTIDE
        if hasattr(r, 'prev_residue') and hasattr(r, 'next_residue'):
            res_flags[k] |= config.R_HAS_SEQ
            if r.prev_residue is not None:
                res_prev[k] = res_index[id(r.prev_residue)]
            if r.next_residue is not None:
                res_next[k] = res_index[id(r.next_residue)]
    adj, sb = [[] for _ in range(n)], np.full(n, -1, np.int32)
    for i, a in enumerate(atoms):
        ob_atom = ic.ob_mol.GetAtomById(ic.bio_to_ob[a])
        for nb in ob.OBAtomAtomIter(ob_atom):
            if nb.GetId() in ic.ob_to_bio:
                adj[i].append(index[ic.ob_to_bio[nb.GetId()]])
        for bond in ob.OBAtomBondIter(ob_atom):                           # utils.py:612-635
            if not (bond.GetBondOrder() == 1 and not bond.IsAromatic()):
                continue
            nbr = bond.GetNbrAtom(ob_atom)
            if nbr.GetAtomicNum() == 1:
                continue
            sb[i] = index[ic.ob_to_bio[nbr.GetId()]]
            break
    bond_off = np.concatenate([[0], np.cumsum([len(x) for x in adj])]).astype(np.int32)
    bond_idx = np.array([j for x in adj for j in x], np.int32)
    h_off = np.concatenate([[0], np.cumsum([len(a.h_coords) for a in atoms])]).astype(np.int32)
    h_xyz = np.array([h for a in atoms for h in a.h_coords], np.float64).reshape(-1, 3)
    rings = ic.biopython_str.rings
    amides = ic.biopython_str.amides
    rkeys, akeys = list(rings), list(amides)
    return PackedComplex(
        xyz=xyz, vdw=[a.vdw_radius for a in atoms], cov=[a.cov_radius for a in atoms], type_mask=tmask, flags=flags,
        res_id=[res_index[id(a.get_parent())] for a in atoms], res_flags=res_flags, res_prev=res_prev, res_next=res_next,
        bond_off=bond_off, bond_idx=bond_idx, h_off=h_off, h_xyz=h_xyz, sb_nbr=sb,
        ring_center=np.array([rings[k]['center'] for k in rkeys], np.float64).reshape(-1, 3),
        ring_normal=np.array([rings[k]['normal'] for k in rkeys], np.float64).reshape(-1, 3),
        ring_res=[res_index[id(rings[k]['residue'])] if rings[k].get('residue') is not None else -1 for k in rkeys],
        # (the reference lists a ring's atoms in molecule order, I:1728-1733; the pack holds the ring PATH, which is what a
        # ring normal is computed along: consecutive atoms bonded)
        ring_atoms=[ring_path_order(np.array([index[a] for a in rings[k]['atoms']], np.int32), adj) for k in rkeys],
        amide_center=np.array([amides[k]['center'] for k in akeys], np.float32).reshape(-1, 3),
        amide_normal=np.array([amides[k]['normal'] for k in akeys], np.float32).reshape(-1, 3),
        amide_res=[res_index[id(amides[k]['residue'])] for k in akeys],
        amide_atoms=np.array([[index[a] for a in amides[k]['atoms']] for k in akeys], np.int32).reshape(-1, 4),
        atom_name=[a.name for a in atoms], element=[a.element for a in atoms],
        serial=[a.serial_number for a in atoms], res_name=[r.resname for r in residues],
        res_seq=[r.id[1] for r in residues], res_icode=[r.id[2] for r in residues],
        res_chain=[r.get_parent().id for r in residues], component_types=dict(ic.component_types), id=ic.id)


class EnsembleComplex:
    """Every model of a multi-model structure (an NMR ensemble, the frames of a simulation) in ONE pass on the GPU, where the
    reference keeps the first model only (P:67-69).  ``filename``: an mmCIF path (``protein_reader.read_mmcif_models``) or a
    tuple ``(pc, xyz [F, n, 3], h_xyz [F, nh, 3])`` of a topology and its models' coordinates.  The other arguments are
    InteractionComplex's.  The topology is kept on the device once; every model gets its own ring / amide geometry and
    ring residues there (arp_set_models) and its own bags, bit-identical to an InteractionComplex run on that model alone.
    ``model(k)`` hands out model k as an InteractionComplex with its results attached (get_contacts, write_json, the CSV
    writers)."""

    def __init__(self, filename, vdw_comp=0.1, interacting=5.0, ph=7.4, device=0, allow_incomplete=False):
        self.allow_incomplete = bool(allow_incomplete)
        if isinstance(filename, tuple):
            pc, xyz, h_xyz = filename
            self.id = pc.id
            self.model_numbers = list(range(1, len(xyz) + 1))
        elif isinstance(filename, (str, os.PathLike)) and str(filename).lower().endswith(('.cif', '.mmcif')):
            from . import protein_reader
            pc, xyz, h_xyz, self.model_numbers = protein_reader.read_mmcif_models(str(filename))
            self.id = os.path.basename(str(filename)).split('.')[0]        # I:51
        else:
            raise NotImplementedError('EnsembleComplex reads mmCIF files (.cif) or (PackedComplex, xyz, h_xyz) tuples')
        self.pc = pc
        self.pc.ensure_labels()
        self.component_types = self.pc.component_types
        self.device = device
        self._ctx = None
        self.params = Parameters(vdw_comp_factor=vdw_comp, interacting_threshold=interacting,
                                 has_hydrogens=bool(np.any(self.pc.flags & config.F_HYDROGEN)) or self.pc.h_xyz.shape[0] > 0, ph=ph)
        self._set_arrays(xyz, h_xyz)
        self._results = None
        self._contact_filter = None      # (sift_any, ctype_mask) of set_contact_filter
        self.persistence = None          # the table of run_persistence and the models it covers
        self.persistence_models = 0
        self.residue_persistence = None  # the table of run_residue_persistence and the models it covers
        self.residue_persistence_models = 0
        self.bridge_persistence = None   # the table of run_water_bridge_persistence, the models it covers and what it was made with
        self.bridge_persistence_models = 0
        self._bridge_persistence_key = None
        self.similarity = None           # the matrix of run_similarity (uint32 [F, F]) and the rows it was made over
        self.similarity_rows = 0
        self.coupling = None             # (features, pairs) of run_coupling, its level and the effective threshold on |phi|
        self.coupling_level = 'atom'
        self.coupling_threshold = None
        self.lifetimes = None            # the table of run_lifetimes, the models it covers and (gap, sift_any, ctype_mask)
        self.lifetimes_models = 0
        self._lifetimes_key = None

    @property
    def n_models(self):
        return int(self.xyz.shape[0])

    def _set_arrays(self, xyz, h_xyz):
        xyz = np.ascontiguousarray(xyz, np.float32)
        h_xyz = np.ascontiguousarray(h_xyz, np.float64).reshape(len(xyz), -1, 3)
        if xyz.ndim != 3 or xyz.shape[1:] != (self.pc.n_atoms, 3) or h_xyz.shape[1] != self.pc.h_xyz.shape[0] or len(xyz) < 1:
            raise ValueError(f'EnsembleComplex: xyz must be [F >= 1, {self.pc.n_atoms}, 3] and h_xyz [F, {self.pc.h_xyz.shape[0]}, 3]')
        self.xyz, self.h_xyz = xyz, h_xyz

    def structure_checks(self):
        """I:109-118 (serial numbers of the topology)."""
        serials = self.pc.serial
        if len(serials) > len(set(serials.tolist())):
            raise AtomSerialError

    def initialize(self):
        """Keep the topology on the GPU and make the models resident, with each model's ring / amide geometry and ring
        residues computed there."""
        from .. import _capi
        incomplete = getattr(self.pc, 'incomplete', ())
        if 'added hydrogens' in incomplete and not self.params.has_hydrogens and self.pc.n_atoms:
            InteractionComplex._incomplete(self, ['hydrogens (the file has none; the reference adds them with OpenBabel, I:99-105)'])
        pc = self.pc
        bad = pc.rings_not_in_path_order()
        if bad:
            raise ValueError(f'ring_atoms of ring(s) {bad[:8]} are not in ring-path order (consecutive atoms are not bonded)')
        if pc.n_amides and (pc.amide_atoms >= 0).all():       # (as compute_plane_geometry: the residue of every amide, I:1554-1559)
            pc.amide_res = amide_majority_residue(pc.res_id, pc.amide_atoms)
        if self._ctx is None:
            self._ctx = _capi.Context(self.device)
            self._ctx.set_sort_after_pass(True)
        self._ctx.set_topology(pc)
        self._ctx.set_models(self.xyz, self.h_xyz)
        self.planes = self._ctx.models_planes()
        self._results = None

    def _incomplete(self, needs):
        InteractionComplex._incomplete(self, needs)

    def set_contact_filter(self, contacts=None, interacting_entities=None):
        """``InteractionComplex.set_contact_filter`` for every model: the next ``run_arpeggio`` fetches the kept atom-atom
        records of all models in one piece and cuts it into the models as it cuts the whole bag (a model's kept records are one
        contiguous range).  The device-reduced tables (``run_persistence`` ...) read the resident bag and do not change."""
        InteractionComplex.set_contact_filter(self, contacts, interacting_entities)

    def set_coordinates(self, xyz, h_xyz):
        """Replace the models (any number of them: the next chunk of a trajectory; numbered 1 ... F); only their coordinates
        go to the GPU."""
        self._set_arrays(xyz, h_xyz)
        self.model_numbers = list(range(1, self.n_models + 1))
        if self._ctx is None:
            self.initialize()
        else:
            self._ctx.set_models(self.xyz, self.h_xyz)
            self.planes = self._ctx.models_planes()
        self._results = None

    def _upload_selection(self, user_selections):
        """The selectors, parsed once on the topology, select the same atoms in each model; returns their indices."""
        pc, F, n = self.pc, self.n_models, self.pc.n_atoms
        if isinstance(user_selections, np.ndarray):
            idx = np.unique(user_selections.astype(np.int64))
        elif user_selections:
            idx = utils.selection_parser(user_selections, pc)
        else:
            idx = np.arange(n, dtype=np.int64)
        if idx.size == 0:                                                   # I:1399-1401
            logging.error('Selection was empty.')
            raise AttributeError('Selection must not be empty.')
        mask = np.zeros(n, np.uint8)
        mask[idx] = 1
        self._ctx.set_selection(np.tile(mask, F))
        return idx

    def run_persistence(self, user_selections, interacting_cutoff, vdw_comp, include_sequence_adjacent, accumulate=False):
        """Contact persistence over the models: the selection handling and the pass of ``run_arpeggio``, then the atom-atom
        records of all models reduced ON THE DEVICE to one row per topology pair (``arpeggio_amd.persistence`` describes the
        table) — and only that table fetched, into ``self.persistence`` (also returned).  No bag is copied to the host:
        ``model(k)`` has no results after this call (``run_arpeggio`` gives those).  ``accumulate=True`` merges the table
        into that of the calls before it, this call's models following theirs (``self.persistence_models`` counts them): a
        trajectory streams through ``set_coordinates`` + ``run_persistence(..., accumulate=True)`` chunk by chunk."""
        from .. import persistence as _persistence
        if self._ctx is None:
            self.initialize()
        self._upload_selection(user_selections)
        self._ctx.run_launch(interacting_cutoff, vdw_comp, include_sequence_adjacent, config.SELECTION_EXPANSION_RADIUS)
        t = self._ctx.models_persistence()
        self._results = None
        if accumulate and self.persistence is not None:
            self.persistence = _persistence.merge(self.persistence, t, self.persistence_models)
            self.persistence_models += self.n_models
        else:
            self.persistence, self.persistence_models = t, self.n_models
        self.stats = self._ctx.stats()
        return self.persistence

    def run_residue_contacts(self, user_selections, interacting_cutoff, vdw_comp, include_sequence_adjacent):
        """The residue-residue contact table of every model: the selection handling and the pass of ``run_arpeggio``, then the
        records of all models folded by residue ON THE DEVICE (``arpeggio_amd.residue_pairs`` describes the table) and only
        that table fetched and cut: a list of F tables with model-local residue ids.  No bag is copied to the host:
        ``model(k)`` has no results after this call (``run_arpeggio`` gives those)."""
        from .. import residue_pairs
        if self._ctx is None:
            self.initialize()
        self._upload_selection(user_selections)
        self._ctx.run_launch(interacting_cutoff, vdw_comp, include_sequence_adjacent, config.SELECTION_EXPANSION_RADIUS)
        t = self._ctx.residue_pairs()
        self._results = None
        self.stats = self._ctx.stats()
        return residue_pairs.split(t, np.arange(self.n_models + 1, dtype=np.int64) * self.pc.n_residues)

    def run_water_bridges(self, user_selections, interacting_cutoff, vdw_comp, include_sequence_adjacent, contacts=('hbond', 'polar'),
                          same_residue=False):
        """Extension beside the mirror: the water-mediated contacts of every model (``InteractionComplex.water_bridges``): the
        selection handling and the pass of ``run_arpeggio``, then ONE join on the device over the records of all models and
        ONE fetch of the table.  A water only meets atoms of its own model, so the rows of a model are one contiguous range:
        the table comes back with topology atom ids and a ``model`` column (0-based, int32), rows ascending by (model, water,
        a, b).  No bag is copied to the host: ``model(k)`` has no results after this call (``run_arpeggio`` gives those).
        Persistence of bridges over the models is ``run_water_bridge_persistence``."""
        from .. import water_bridges as wb
        if self._ctx is None:
            self.initialize()
        self._upload_selection(user_selections)
        self._ctx.run_launch(interacting_cutoff, vdw_comp, include_sequence_adjacent, config.SELECTION_EXPANSION_RADIUS)
        t = self._ctx.water_bridges(wb.mask(contacts), wb.SAME_RESIDUE if same_residue else 0)
        self._results = None
        self.stats = self._ctx.stats()
        n = self.pc.n_atoms
        model = (t['water'] // n).astype(np.int32)
        out = {k: ((t[k] - model * n).astype(np.int32) if k in ('water', 'a', 'b') else t[k]) for k, _ in wb.COLUMNS}
        out['model'] = model
        return out

    def run_networks(self, user_selections, interacting_cutoff, vdw_comp, include_sequence_adjacent, contacts=None,
                     interacting_entities=None, level='atom'):
        """Extension beside the mirror: the interaction networks of every model (``InteractionComplex.networks``): the
        selection handling and the pass of ``run_arpeggio``, then ONE launch on the device over the records of all models and
        ONE fetch each of the labels and of the table.  No record joins two models, so no component spans them: ``label``
        comes back as int32 [F, n] (``level='residue'``: [F, residues of the topology]) in topology ids, -1 kept, and the table
        with topology ids in ``root`` and a ``model`` column (0-based, int32), rows ascending by (model, root).  No bag is
        copied to the host: ``model(k)`` has no results after this call (``run_arpeggio`` gives those)."""
        from .. import contact_filter
        if level not in ('atom', 'residue'):
            raise ValueError("run_networks: level must be 'atom' or 'residue'")
        sift_any, ctype_mask = contact_filter.masks(contacts, interacting_entities)
        if self._ctx is None:
            self.initialize()
        self._upload_selection(user_selections)
        self._ctx.run_launch(interacting_cutoff, vdw_comp, include_sequence_adjacent, config.SELECTION_EXPANSION_RADIUS)
        label, t = self._ctx.networks(sift_any, ctype_mask, level == 'residue')
        self._results = None
        self.stats = self._ctx.stats()
        F = self.n_models
        n = len(label) // F
        label = label.reshape(F, n)
        label = np.where(label >= 0, label - (np.arange(F, dtype=np.int32) * n)[:, None], -1).astype(np.int32)
        model = (t['root'] // max(n, 1)).astype(np.int32)
        out = dict(t, root=(t['root'] - model * n).astype(np.int32))
        out['model'] = model
        return label, out

    def run_residue_persistence(self, user_selections, interacting_cutoff, vdw_comp, include_sequence_adjacent, accumulate=False):
        """Residue contact persistence over the models — a residue contact-frequency map: the selection handling and the pass
        of ``run_persistence``, then the records of all five bags of all models reduced ON THE DEVICE to one row per pair of
        topology residues (``arpeggio_amd.residue_persistence`` describes the table) — and only that table fetched, into
        ``self.residue_persistence`` (also returned).  No bag is copied to the host: ``model(k)`` has no results after this
        call (``run_arpeggio`` gives those).  ``accumulate=True`` merges the table into that of the calls before it, this
        call's models following theirs (``self.residue_persistence_models`` counts them), as ``run_persistence`` does for the
        atom table."""
        from .. import residue_persistence as _respersist
        if self._ctx is None:
            self.initialize()
        self._upload_selection(user_selections)
        self._ctx.run_launch(interacting_cutoff, vdw_comp, include_sequence_adjacent, config.SELECTION_EXPANSION_RADIUS)
        t = self._ctx.models_residue_persistence()
        self._results = None
        if accumulate and self.residue_persistence is not None:
            self.residue_persistence = _respersist.merge(self.residue_persistence, t, self.residue_persistence_models)
            self.residue_persistence_models += self.n_models
        else:
            self.residue_persistence, self.residue_persistence_models = t, self.n_models
        self.stats = self._ctx.stats()
        return self.residue_persistence

    def run_water_bridge_persistence(self, user_selections, interacting_cutoff, vdw_comp, include_sequence_adjacent,
                                     contacts=('hbond', 'polar'), same_residue=False, level='atom', accumulate=False):
        """Extension beside the mirror: water-bridge persistence over the models — in what fraction of the models a water
        bridges two atoms (``level='atom'``) or two residues (``level='residue'``), through how many waters and how tightly:
        the selection handling and the pass of ``run_water_bridges``, then the bridges of all models joined and folded ON THE
        DEVICE to one row per topology pair (``arpeggio_amd.bridge_persistence`` describes the table) — and only that table
        fetched, into ``self.bridge_persistence`` (also returned).  ``contacts`` and ``same_residue`` are those of
        ``run_water_bridges``.  No bag is copied to the host: ``model(k)`` has no results after this call.
        ``accumulate=True`` merges the table into that of the calls before it, this call's models following theirs
        (``self.bridge_persistence_models`` counts them), as ``run_residue_persistence`` does; ``ValueError`` when the
        contacts, ``same_residue`` or the level differ from those of the accumulated table."""
        from .. import _capi, bridge_persistence as _bp, water_bridges as wb
        if level not in _bp.LEVELS:
            raise ValueError(f"run_water_bridge_persistence: level must be 'atom' or 'residue', not {level!r}")
        key = (wb.mask(contacts), bool(same_residue), level)
        merging = accumulate and self.bridge_persistence is not None
        if merging and key != self._bridge_persistence_key:
            raise ValueError('run_water_bridge_persistence: accumulate=True with other contacts, same_residue or level than the '
                             'accumulated table was made with')
        if self._ctx is None:
            self.initialize()
        self._upload_selection(user_selections)
        self._ctx.run_launch(interacting_cutoff, vdw_comp, include_sequence_adjacent, config.SELECTION_EXPANSION_RADIUS)
        flags = (wb.SAME_RESIDUE if same_residue else 0) | (_capi.WBP_BY_RESIDUE if level == 'residue' else 0)
        t = self._ctx.models_water_bridge_persistence(key[0], flags)
        self._results = None
        if merging:
            self.bridge_persistence = _bp.merge(self.bridge_persistence, t, self.bridge_persistence_models)
            self.bridge_persistence_models += self.n_models
        else:
            self.bridge_persistence, self.bridge_persistence_models, self._bridge_persistence_key = t, self.n_models, key
        self.stats = self._ctx.stats()
        return self.bridge_persistence

    def write_bridge_persistence(self, wd):
        """'<id>.bridgepersist' in ``wd``: the table of ``run_water_bridge_persistence`` as CSV."""
        from .. import bridge_persistence as _bp
        if self.bridge_persistence is None:
            raise AttributeError('write_bridge_persistence: run_water_bridge_persistence first')
        return _bp.write_bridge_persistence(wd, self.id, self.bridge_persistence, self.pc, self.component_types)

    def run_similarity(self, user_selections, interacting_cutoff, vdw_comp, include_sequence_adjacent, contacts=None, classes=(),
                       interacting_entities=None, level='atom'):
        """Extension beside the mirror: interaction-fingerprint similarity between the models — which models share their
        contacts: the selection handling and the pass of ``run_persistence``, then the records of all models turned ON THE
        DEVICE into one bit per (model, row, plane) and multiplied there to ``inter`` uint32 [F, F], the features two models
        share (``arpeggio_amd.similarity`` describes it and derives Tanimoto, distance and medoid) — and only that matrix
        fetched, into ``self.similarity`` (also returned).  A row is a topology atom pair (``level='atom'``) or a topology
        residue pair over all five bags (``level='residue'``).  ``contacts`` / ``classes`` name the planes
        (``similarity.planes``: ``None`` = every contact but bare proximity; the ring / amide classes exist at residue level
        only); ``interacting_entities`` names the kinds of entities whose atom-atom records take part
        (``contact_filter.masks``; ``None`` = all).  No bag is copied to the host: ``model(k)`` has no results after this
        call.  There is no ``accumulate``: the block of the matrix between two chunks of a trajectory needs the records of
        both chunks resident, so a streamed trajectory is out of scope — make the models of interest resident together (up
        to ``similarity.MAX_MODELS``)."""
        from .. import contact_filter, similarity as _sim
        if level not in ('atom', 'residue'):
            raise ValueError(f"run_similarity: level must be 'atom' or 'residue', not {level!r}")
        mask = _sim.planes(contacts, classes)
        if level == 'atom' and mask & ~_sim.ATOM_PLANES:
            raise ValueError("run_similarity: the ring / amide classes are planes of level='residue' only")
        ctype_mask = contact_filter.masks(None, interacting_entities)[1]
        if self._ctx is None:
            self.initialize()
        self._upload_selection(user_selections)
        self._ctx.run_launch(interacting_cutoff, vdw_comp, include_sequence_adjacent, config.SELECTION_EXPANSION_RADIUS)
        self.similarity = self._ctx.models_similarity(mask, ctype_mask, by_residue=level == 'residue')
        self._results = None
        self.stats = self._ctx.stats()
        self.similarity_rows = self.stats['sim_rows']
        return self.similarity

    def write_similarity(self, wd):
        """'<id>.modelsim' in ``wd``: the matrix of ``run_similarity`` as CSV, one line per pair of models (0-based)."""
        from .. import similarity as _sim
        if self.similarity is None:
            raise AttributeError('write_similarity: run_similarity first')
        return _sim.write_similarity(wd, self.id, self.similarity)

    def run_coupling(self, user_selections, interacting_cutoff, vdw_comp, include_sequence_adjacent, contacts=None, classes=(),
                     interacting_entities=None, level='atom', min_occupancy=0.05, max_occupancy=0.95, min_abs_phi=0.7,
                     max_pairs=1 << 20):
        """Extension beside the mirror: contact coupling over the models — which contacts form and break together: the
        selection handling and the pass of ``run_persistence``, then the records of all models turned ON THE DEVICE into one
        bit per (contact, model), the contacts whose occupancy lies in ``min_occupancy`` ... ``max_occupancy`` correlated
        pairwise there, and only the pairs with \\|phi\\| >= ``min_abs_phi`` fetched (``arpeggio_amd.coupling`` describes the
        two tables and derives phi, the Jaccard index and the groups of contacts that switch together), into
        ``self.coupling`` = ``(features, pairs)`` (also returned).  A contact is a topology atom pair (``level='atom'``) or a
        topology residue pair over all five bags (``level='residue'``); ``contacts`` / ``classes`` /
        ``interacting_entities`` are those of ``run_similarity``.  The occupancies become counts of models by ceil and floor,
        clipped to 1 ... F - 1 (``coupling.counts``); the threshold becomes ``coupling.phi2_q(min_abs_phi)``, whose effective
        value is kept in ``self.coupling_threshold``.  More kept pairs than ``max_pairs``: ``NativeLibraryError`` whose
        ``n_pairs`` is their exact number.  No bag is copied to the host: ``model(k)`` has no results after this call.
        There is no ``accumulate``: the threshold is not additive over the chunks of a trajectory."""
        from .. import contact_filter, coupling as _cp, similarity as _sim
        if level not in _cp.LEVELS:
            raise ValueError(f"run_coupling: level must be 'atom' or 'residue', not {level!r}")
        mask = _sim.planes(contacts, classes)
        if level == 'atom' and mask & ~_sim.ATOM_PLANES:
            raise ValueError("run_coupling: the ring / amide classes are planes of level='residue' only")
        ctype_mask = contact_filter.masks(None, interacting_entities)[1]
        lo, hi = _cp.counts(min_occupancy, max_occupancy, self.n_models)
        if lo > hi:
            raise ValueError('run_coupling: no count of models lies between min_occupancy and max_occupancy')
        q, effective = _cp.phi2_q(min_abs_phi)
        if self._ctx is None:
            self.initialize()
        self._upload_selection(user_selections)
        self._ctx.run_launch(interacting_cutoff, vdw_comp, include_sequence_adjacent, config.SELECTION_EXPANSION_RADIUS)
        self.coupling = self._ctx.models_coupling(mask, ctype_mask, by_residue=level == 'residue', min_count=lo, max_count=hi, phi2_q=q,
                                                  max_pairs=max_pairs)
        self.coupling_level, self.coupling_threshold = level, effective
        self._results = None
        self.stats = self._ctx.stats()
        return self.coupling

    def write_coupling(self, wd):
        """'<id>.coupling' in ``wd``: the kept pairs of ``run_coupling`` as CSV."""
        from .. import coupling as _cp
        if self.coupling is None:
            raise AttributeError('write_coupling: run_coupling first')
        return _cp.write_coupling(wd, self.id, self.coupling[0], self.coupling[1], self.pc, self.n_models, self.coupling_level,
                                  self.component_types)

    def run_lifetimes(self, user_selections, interacting_cutoff, vdw_comp, include_sequence_adjacent, gap=0, contacts=None,
                      interacting_entities=None, accumulate=False):
        """Extension beside the mirror: contact lifetimes over the models — how long a contact lasts along the ordered axis of
        the models (for a trajectory streamed through ``set_coordinates``, model f is time) and how often it forms and breaks:
        the selection handling and the pass of ``run_persistence``, then the atom-atom records of all models reduced ON THE
        DEVICE to one row per topology pair with its intervals of presence (``arpeggio_amd.lifetimes`` describes the table) —
        and only that table fetched, into ``self.lifetimes`` (also returned).  ``gap``: models of absence tolerated inside an
        interval; ``contacts`` / ``interacting_entities`` name the records that take part (``contact_filter.masks``; ``None``
        = all).  No bag is copied to the host: ``model(k)`` has no results after this call.  ``accumulate=True`` merges the
        table EXACTLY into that of the calls before it, this call's models following theirs (``self.lifetimes_models`` counts
        them); ``ValueError`` when ``gap`` or the masks differ from those of the accumulated table."""
        from .. import contact_filter, lifetimes as _lt
        key = (_lt.check_gap(gap),) + contact_filter.masks(contacts, interacting_entities)
        merging = accumulate and self.lifetimes is not None
        if merging and key != self._lifetimes_key:
            raise ValueError('run_lifetimes: accumulate=True with another gap, other contacts or interacting entities than the '
                             'accumulated table was made with')
        if self._ctx is None:
            self.initialize()
        self._upload_selection(user_selections)
        self._ctx.run_launch(interacting_cutoff, vdw_comp, include_sequence_adjacent, config.SELECTION_EXPANSION_RADIUS)
        t = self._ctx.models_lifetimes(*key)
        self._results = None
        if merging:
            self.lifetimes = _lt.merge(self.lifetimes, t, self.lifetimes_models, key[0])
            self.lifetimes_models += self.n_models
        else:
            self.lifetimes, self.lifetimes_models, self._lifetimes_key = t, self.n_models, key
        self.stats = self._ctx.stats()
        return self.lifetimes

    def write_lifetimes(self, wd):
        """'<id>.lifetimes' in ``wd``: the table of ``run_lifetimes`` as CSV."""
        from .. import lifetimes as _lt
        if self.lifetimes is None:
            raise AttributeError('write_lifetimes: run_lifetimes first')
        return _lt.write_lifetimes(wd, self.id, self.lifetimes, self.pc, self.lifetimes_models, self.component_types)

    def run_arpeggio(self, user_selections, interacting_cutoff, vdw_comp, include_sequence_adjacent):
        """I:329-347 on every model: the selectors are parsed once on the topology and select the same atoms in each model."""
        if self._ctx is None:
            self.initialize()
        pc, ctx, F, n = self.pc, self._ctx, self.n_models, self.pc.n_atoms
        idx = self._upload_selection(user_selections)
        per_model = ctx.run_models(interacting_cutoff, vdw_comp, include_sequence_adjacent, config.SELECTION_EXPANSION_RADIUS,
                                   contact_filter=self._contact_filter)
        masks = ctx.make_selection_masks()
        R, A = pc.n_rings, pc.n_amides
        self._results = []
        for f in range(F):
            plus = np.nonzero(masks['plus'][f * n:(f + 1) * n])[0]
            self._results.append(dict(
                bags=per_model[f], selection=idx, selection_plus=plus, selection_plus_residues=np.unique(pc.res_id[plus]),
                selection_ring_ids=set(np.nonzero(masks['ring_sel'][f * R:(f + 1) * R])[0].tolist()),
                selection_plus_ring_ids=set(np.nonzero(masks['ring_plus'][f * R:(f + 1) * R])[0].tolist()),
                selection_amide_ids=set(np.nonzero(masks['amide_sel'][f * A:(f + 1) * A])[0].tolist()),
                selection_plus_amide_ids=set(np.nonzero(masks['amide_plus'][f * A:(f + 1) * A])[0].tolist())))
        for f in range(F):
            self.model(f)._check_incomplete_after_run()
        self.stats = ctx.stats()

    def model_pack(self, k):
        """Model k (0-based) as a PackedComplex: the topology with model k's coordinates and plane geometry."""
        import copy
        if self._ctx is None:
            self.initialize()
        q = copy.copy(self.pc)
        q.xyz, q.h_xyz = self.xyz[k], self.h_xyz[k]
        p = self.planes
        q.ring_center, q.ring_normal, q.ring_res = p['ring_center'][k], p['ring_normal'][k], p['ring_res'][k]
        q.amide_center, q.amide_normal = p['amide_center'][k], p['amide_normal'][k]
        if len(q.amide_atoms) and (q.amide_atoms >= 0).all():
            q.amide_res = amide_majority_residue(q.res_id, q.amide_atoms)
        q.plane_geometry_pending = False
        return q

    def model(self, k):
        """Model k (0-based) as an InteractionComplex with the results of the last run_arpeggio attached: get_contacts,
        write_json and the CSV writers work on it unchanged (it holds no GPU context of its own)."""
        ic = InteractionComplex(self.model_pack(k), self.params.vdw_comp_factor, self.params.interacting_threshold, self.params.ph,
                                self.device, self.allow_incomplete)
        ic.id = self.id if self.n_models == 1 else f'{self.id}_model{self.model_numbers[k]}'
        ic._contact_filter = self._contact_filter
        if self._results is not None:
            r = self._results[k]
            ic._bags = r['bags']
            for key in ('selection', 'selection_plus', 'selection_plus_residues', 'selection_ring_ids', 'selection_plus_ring_ids',
                        'selection_amide_ids', 'selection_plus_amide_ids'):
                setattr(ic, key, r[key])
        return ic
