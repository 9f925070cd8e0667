"""The class graft, stated once. Every fused block reaches the reference the same way: a subclass of one of the reference's classes
is made at run time with one method overridden, and a built module's `__class__` is set to it.

A seam is the pair (owning module's name, the name of its factory function there): ("guassianhand_amd.attention",
"fused_self_attn_cls"). The factory is a module-level function `factory(base, *options)` that calls `graft`; it is what the config
modules (tgs_renderer and the like) and `swap` call, and what a pickle calls again on load. The registry is per seam: grafts stack
(the attention block over the attention core, the fused trunk over a tgs_renderer variant), and a class one seam made is an ordinary
base to every other.

A made class carries `_gh_seam`, `_gh_base` and `_gh_options`, and a `__reduce_ex__` that rebuilds the class chain instead of naming
it: the first recorded base that no seam made pickles by reference, as any class does, and above it each (module, factory, options)
is imported and called in order. pickle and copy.deepcopy of a grafted module therefore give an instance of the identical class, in
a process that has imported nothing of this package as well.

Not covered: the two instance hooks, plane.fuse_plane_fetch and uvd.fuse_get_uvd, set attributes on an object, not a class.
Pickling a whole renderer that carries them is out of scope here."""
from importlib import import_module

_made = {}                                                        # seam -> {(base, options): the made class}


def graft(seam, base, overrides, what=None, *, options=(), doc=None):
    """The cached subclass of `base` carrying `overrides`, for this seam and these options. It keeps the base's name, lives in the
    seam's module and documents itself as "<base> with the MI355X <what>" (or `doc`)."""
    classes = _made.setdefault(seam, {})
    if (base, options) not in classes:
        body = {"__module__": seam[0], "__doc__": doc or f"{base.__module__}.{base.__name__} with the MI355X {what}",
                "__reduce_ex__": _reduce_ex, "_gh_seam": seam, "_gh_base": base, "_gh_options": options}
        classes[(base, options)] = type(base.__name__, (base,), {**body, **overrides})
    return classes[(base, options)]


def is_grafted(seam, cls) -> bool:
    """Whether `cls` is exactly a class this seam made (a subclass of one is not)."""
    return vars(cls).get("_gh_seam") == seam


def swap(seam, module, *options):
    """Set `module.__class__` to the seam's graft of its class, unless it is that already. Where it is the seam's class with other
    options, the graft is made of the recorded base instead. Returns the module."""
    cls = type(module)
    if is_grafted(seam, cls):
        if cls._gh_options == options:
            return module
        cls = cls._gh_base
    module.__class__ = getattr(import_module(seam[0]), seam[1])(cls, *options)
    return module


def _reduce_ex(self, protocol):
    chain, cls = [], type(self)
    while "_gh_seam" in vars(cls):
        chain.append((*cls._gh_seam, cls._gh_options))
        cls = cls._gh_base
    return _rebuild, (cls, tuple(reversed(chain))), self.__dict__


def _rebuild(cls, chain):
    for module, factory, options in chain:
        cls = getattr(import_module(module), factory)(cls, *options)
    return cls.__new__(cls)
