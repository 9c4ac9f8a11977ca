"""
Classes for dealing with biological sequences; stands where lib/bx/seq/__init__.py of the reference stands.  ``bx.seq.twobit``,
``bx.seq.seq``, ``bx.seq.fasta`` and ``bx.seq.nib`` are served by this package; the other ``bx.seq`` modules (``core``, ``qdna``, ... and
the names the reference re-exports from ``core``) resolve to an installed bx-python.
"""
from pkgutil import extend_path

__path__ = extend_path(__path__, __name__)
