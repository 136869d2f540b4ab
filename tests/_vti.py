"""A reader for the files beat.output writes, independent of the writer (test_output_cpu.py, test_output_gpu.py): the XML of a .vti
up to the ``_`` of its appended section, then per array a UInt64 byte count and the bytes; the DataSet entries of a .pvd."""
import re
import xml.etree.ElementTree as ET
from types import SimpleNamespace

import numpy as np

_TYPES = {"Float32": np.dtype("<f4"), "Float64": np.dtype("<f8")}


def read_vti(path):
    """extent (6 ints), origin, spacing (3 floats), arrays name -> (nz, ny, nx) array, offsets name -> int, scalars."""
    blob = open(path, "rb").read()
    m = re.search(rb'<AppendedData encoding="raw">\s*_', blob)
    assert m is not None, "no raw appended section"
    head, data = blob[: m.start()], blob[m.end():]
    assert data.endswith(b"\n  </AppendedData>\n</VTKFile>\n")
    root = ET.fromstring(head + b"</VTKFile>")
    assert root.tag == "VTKFile" and root.attrib["type"] == "ImageData" and root.attrib["byte_order"] == "LittleEndian"
    assert root.attrib["header_type"] == "UInt64"
    image = root.find("ImageData")
    piece = image.find("Piece")
    extent = [int(w) for w in image.attrib["WholeExtent"].split()]
    assert piece.attrib["Extent"] == image.attrib["WholeExtent"]
    shape = (extent[5] - extent[4] + 1, extent[3] - extent[2] + 1, extent[1] - extent[0] + 1)
    arrays, offsets = {}, {}
    point_data = piece.find("PointData")
    for da in point_data.findall("DataArray"):
        assert da.attrib["format"] == "appended"
        off = int(da.attrib["offset"])
        nbytes = int(np.frombuffer(data, dtype="<u8", count=1, offset=off)[0])
        dt = _TYPES[da.attrib["type"]]
        assert nbytes == int(np.prod(shape)) * dt.itemsize
        arrays[da.attrib["Name"]] = np.frombuffer(data, dtype=dt, count=nbytes // dt.itemsize, offset=off + 8).reshape(shape)
        offsets[da.attrib["Name"]] = off
    return SimpleNamespace(extent=extent, origin=[float(w) for w in image.attrib["Origin"].split()],
                           spacing=[float(w) for w in image.attrib["Spacing"].split()], arrays=arrays, offsets=offsets,
                           scalars=point_data.attrib["Scalars"])


def read_pvd(path):
    """[(time, file name), ...]"""
    root = ET.parse(path).getroot()
    assert root.tag == "VTKFile" and root.attrib["type"] == "Collection"
    return [(float(d.attrib["timestep"]), d.attrib["file"]) for d in root.find("Collection").findall("DataSet")]
