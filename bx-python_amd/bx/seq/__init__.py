"""
Classes for dealing with biological sequences; stands where lib/bx/seq/__init__.py of the reference stands.  Only ``bx.seq.twobit``
is served by this package; the other ``bx.seq`` modules (``core``, ``nib``, ``qdna``, ... and the names the reference re-exports
from ``core``) resolve to an installed bx-python.
"""
from pkgutil import extend_path

__path__ = extend_path(__path__, __name__)
