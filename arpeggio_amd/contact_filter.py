"""Which atom-atom records a caller wants: the two masks of ``Context.fetch_packed_filtered`` (arp_contacts_filter_launch) by
name, two presets, and the same predicate on the host.

A record is kept when ``(sift & sift_any) != 0`` and bit ``ctype`` of ``ctype_mask`` is set: at least one of the named
contacts, between interacting entities of one of the named kinds.  There is no distance term (a smaller cutoff is another
pass) and no "none of these" term; the five ladder bits (clash, covalent, vdw_clash, vdw, proximal) exclude each other, so
"everything but bare proximity" is every bit but ``proximal`` (``SPECIFIC``).  Pure host code: no GPU, no native library.
"""
from __future__ import annotations

import numpy as np

from .core import config

SIFT_ALL = (1 << len(config.SIFT_NAMES)) - 1                  # ARP_FILTER_SIFT_ALL
CTYPE_ALL = (1 << len(config.CONTACT_TYPE_NAMES)) - 1         # ARP_FILTER_CTYPE_ALL


def _mask(names, known, what):
    if names is None:
        return (1 << len(known)) - 1
    if isinstance(names, str):
        names = [names]
    names = list(names)
    if not names:
        raise ValueError(f'contact_filter.masks: an empty list of {what} keeps nothing (None means all)')
    m = 0
    for nm in names:
        if nm not in known:
            raise ValueError(f'contact_filter.masks: unknown {what} name {nm!r} (known: {", ".join(known)})')
        m |= 1 << known.index(nm)
    return m


def masks(contacts=None, interacting_entities=None):
    """``(sift_any, ctype_mask)`` for the contacts named in ``contacts`` (``config.SIFT_NAMES``: 'hbond', 'ionic', ...) between
    the kinds of entities named in ``interacting_entities`` (``config.CONTACT_TYPE_NAMES``: 'INTER', ...).  ``None`` means
    all; an unknown name or an empty list raises ``ValueError``."""
    return (_mask(contacts, config.SIFT_NAMES, 'contact'),
            _mask(interacting_entities, config.CONTACT_TYPE_NAMES, 'interacting-entities'))


# every contact but bare proximity, between any entities
SPECIFIC = (SIFT_ALL & ~(1 << config.SIFT_NAMES.index('proximal')), CTYPE_ALL)
# the records of the reference's '<id>_bs_contacts.csv' (interactions.py:166): any contact, four of the seven entity kinds
BINDING_SITE = masks(None, ('INTER', 'INTRA_SELECTION', 'SELECTION_WATER', 'WATER_WATER'))


def keep(sift, ctype, sift_any, ctype_mask):
    """The predicate on arrays: a bool array, True where the record is kept."""
    sift = np.asarray(sift).astype(np.uint32)
    ctype = np.asarray(ctype).astype(np.uint32)
    return ((sift & np.uint32(sift_any)) != 0) & (((np.uint32(ctype_mask) >> np.minimum(ctype, 31)) & 1) != 0)


def apply(bag, sift_any, ctype_mask):
    """The kept records of an atom-atom records bag (a dict with the columns i, j, dist, sift, ctype; a ``RowsBag`` gives its
    ``i``) as a new dict of those five columns, order unchanged — what ``fetch_packed_filtered`` delivers, made on the host
    from the whole bag."""
    m = keep(bag['sift'], bag['ctype'], sift_any, ctype_mask)
    return {k: np.asarray(bag[k])[m] for k in ('i', 'j', 'dist', 'sift', 'ctype')}
