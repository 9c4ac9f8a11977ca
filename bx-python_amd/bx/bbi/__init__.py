"""
Support for UCSC "big binary indexed" files; mirrors lib/bx/bbi/__init__.py of the reference (a docstring, no re-exports).
Only ``bx.bbi.bigwig_file`` is served by this package; the other ``bx.bbi`` modules resolve to an installed bx-python.
"""
from pkgutil import extend_path

__path__ = extend_path(__path__, __name__)
