"""Mirror of the reference's ``sunerf/baseline/reprojection.py``: its import path and its three public names on the device
kernels of ``sunerf_hip.reprojection``.

Kept: the names, the order of arguments, the default map shape (1024, 2048), ``load_views``' 10-degree grid of observers at
1 AU and its ``((lat, lon), view)`` pairs.  Changed: the inputs are :class:`sunerf_hip.observations.View` objects (images on
the device with pose and pixel grid) instead of sunpy ``Map`` s, the results are device tensors instead of ``Map`` s, angles are
plain radians and distances plain solar radii (astropy quantities where astropy is importable), and there is no
``multiprocessing.Pool``: all observers of ``load_views`` come from one kernel launch.

Not built: sunpy ``Map`` inputs and FITS headers, ``synoptic=True``, ``obstime`` (the map is in the frame of the rays and all
views are taken as simultaneous) and ``create_new_observer`` (an observer is a pose plus a pixel grid:
:class:`sunerf_hip.reprojection.Observer`).
"""
from sunerf_hip.observations import AU_IN_SOLAR_RADII, resampled_grid
from sunerf_hip.reprojection import synchronic_map


def create_heliographic_map(*views, shape_out=(1024, 2048), Rs_per_ds=1.0, **kw):
    """The synchronic map of ``views`` (reprojection.py:52-95) as a :class:`sunerf_hip.reprojection.SynchronicMap`."""
    return synchronic_map(list(views), shape=shape_out, Rs_per_ds=Rs_per_ds, **kw)


def transform(*views, lat, lon, distance, grid=None, tx=None, ty=None, center=None, off_disk=None, Rs_per_ds=1.0):
    """``views`` seen from a new viewpoint (reprojection.py:98-125): ``(H, W, C)`` on the pixel grid ``grid`` (plate-scale dict)
    or ``tx`` / ``ty``; default: the grid of the first view."""
    h_map = create_heliographic_map(*views, Rs_per_ds=Rs_per_ds)
    if grid is None and tx is None:
        tx, ty = views[0].tx, views[0].ty
    return h_map.reproject(lat, lon, distance, grid=grid, tx=tx, ty=ty, center=center, off_disk=off_disk)


def load_views(*views, strides=10, resolution=None, distance=AU_IN_SOLAR_RADII, off_disk=None, Rs_per_ds=1.0):
    """Yields ``((lat, lon) [deg], view (H, W, C))`` for the viewpoints ``mgrid[-90:91:strides, 0:361:strides]``
    (reprojection.py:128-168) on the pixel grid of the first view; ``resolution`` = (H, W) resamples that grid over the same
    field of view (the reference's ``resample``; the first view then needs a plate-scale grid)."""
    h_map = create_heliographic_map(*views, Rs_per_ds=Rs_per_ds)
    first = views[0]
    if resolution is not None:
        if first.grid is None:
            raise ValueError('load_views: resolution= needs a first view with a plate-scale grid')
        yield from h_map.view_grid(strides, distance, grid=resampled_grid(first.grid, resolution), off_disk=off_disk)
    else:
        yield from h_map.view_grid(strides, distance, tx=first.tx, ty=first.ty, off_disk=off_disk)
