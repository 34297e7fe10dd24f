"""glTF 2.0 binary (.glb) files with numpy and the standard library: what examples/full_res_3d_viz.py writes in place
of the reference's interactive VTK window, and a reader for the tests.

Scene collects nodes, meshes, materials and one binary buffer.  Every POSITION accessor carries min and max (the
specification requires them); indices are uint32; materials are double-sided with a base colour and, optionally, a
PNG texture (dfl_amd.png) sampled NEAREST.  Chunks are padded to 4 bytes (JSON with spaces, BIN with zeros)."""
import json
import struct

import numpy as np

from . import png

MAGIC, VERSION = 0x46546C67, 2          # b'glTF'
JSON_CHUNK, BIN_CHUNK = 0x4E4F534A, 0x004E4942
FLOAT, UINT32 = 5126, 5125
ARRAY_BUFFER, ELEMENT_ARRAY_BUFFER = 34962, 34963
TRIANGLES, LINES = 4, 1
NEAREST = 9728
_TYPES = {1: 'SCALAR', 2: 'VEC2', 3: 'VEC3'}
_NP = {FLOAT: np.float32, UINT32: np.uint32}


class Scene:
    def __init__(self):
        self.doc = {'asset': {'version': '2.0', 'generator': 'dfl_amd.gltf'}, 'scene': 0, 'scenes': [{'nodes': []}],
                    'nodes': [], 'meshes': [], 'materials': [], 'accessors': [], 'bufferViews': []}
        self._bin = bytearray()

    def _view(self, data, target=None):
        while len(self._bin) % 4:
            self._bin.append(0)
        view = {'buffer': 0, 'byteOffset': len(self._bin), 'byteLength': len(data)}
        if target is not None:
            view['target'] = target
        self._bin += data
        self.doc['bufferViews'].append(view)
        return len(self.doc['bufferViews']) - 1

    def accessor(self, array, component, target=None, bounds=False):
        a = np.ascontiguousarray(array, dtype=_NP[component])
        cols = 1 if a.ndim == 1 else a.shape[1]
        acc = {'bufferView': self._view(a.tobytes(), target), 'componentType': component, 'count': int(a.shape[0]),
               'type': _TYPES[cols]}
        if bounds:
            m = a.reshape(a.shape[0], cols)
            acc['min'] = [float(v) for v in m.min(0)]
            acc['max'] = [float(v) for v in m.max(0)]
        self.doc['accessors'].append(acc)
        return len(self.doc['accessors']) - 1

    def material(self, name, rgb, texture_rgb=None):
        """A double-sided material of base colour rgb (0..1); texture_rgb [H, W, 3] uint8 becomes its PNG texture."""
        m = {'name': name, 'doubleSided': True,
             'pbrMetallicRoughness': {'baseColorFactor': [float(c) for c in rgb] + [1.0], 'metallicFactor': 0.0,
                                      'roughnessFactor': 1.0}}
        if texture_rgb is not None:
            d = self.doc
            d.setdefault('images', []).append({'bufferView': self._view(png.encode(texture_rgb)), 'mimeType': 'image/png'})
            d.setdefault('samplers', []).append({'magFilter': NEAREST, 'minFilter': NEAREST})
            d.setdefault('textures', []).append({'source': len(d['images']) - 1, 'sampler': len(d['samplers']) - 1})
            m['pbrMetallicRoughness']['baseColorTexture'] = {'index': len(d['textures']) - 1}
        self.doc['materials'].append(m)
        return len(self.doc['materials']) - 1

    def mesh(self, name, positions, indices, material, normals=None, texcoords=None, mode=TRIANGLES):
        attr = {'POSITION': self.accessor(positions, FLOAT, ARRAY_BUFFER, bounds=True)}
        if normals is not None:
            attr['NORMAL'] = self.accessor(normals, FLOAT, ARRAY_BUFFER)
        if texcoords is not None:
            attr['TEXCOORD_0'] = self.accessor(texcoords, FLOAT, ARRAY_BUFFER)
        prim = {'attributes': attr, 'mode': mode, 'material': material}
        if indices is not None:
            prim['indices'] = self.accessor(np.asarray(indices).reshape(-1), UINT32, ELEMENT_ARRAY_BUFFER)
        self.doc['meshes'].append({'name': name, 'primitives': [prim]})
        return len(self.doc['meshes']) - 1

    def node(self, name, mesh=None, translation=None, scale=None):
        n = {'name': name}
        if mesh is not None:
            n['mesh'] = mesh
        if translation is not None:
            n['translation'] = [float(v) for v in translation]
        if scale is not None:
            n['scale'] = [float(v) for v in scale]
        self.doc['nodes'].append(n)
        self.doc['scenes'][0]['nodes'].append(len(self.doc['nodes']) - 1)
        return len(self.doc['nodes']) - 1

    def encode(self):
        doc = dict(self.doc)
        if self._bin:
            doc['buffers'] = [{'byteLength': len(self._bin)}]
        js = json.dumps(doc, separators=(',', ':')).encode()
        js += b' ' * (-len(js) % 4)
        chunks = struct.pack('<II', len(js), JSON_CHUNK) + js
        if self._bin:
            b = bytes(self._bin) + b'\0' * (-len(self._bin) % 4)
            chunks += struct.pack('<II', len(b), BIN_CHUNK) + b
        return struct.pack('<III', MAGIC, VERSION, 12 + len(chunks)) + chunks

    def write(self, path):
        with open(path, 'wb') as f:
            f.write(self.encode())


class Glb:
    """A parsed .glb: doc (the JSON), bin (the BIN chunk), and accessors / images / nodes by name as numpy."""

    def __init__(self, data):
        if isinstance(data, str):
            with open(data, 'rb') as f:
                data = f.read()
        magic, version, length = struct.unpack_from('<III', data, 0)
        if magic != MAGIC or version != VERSION or length != len(data):
            raise ValueError('not a glTF 2.0 binary file')
        self.chunk_lengths = []
        pos, self.bin = 12, b''
        while pos < length:
            n, kind = struct.unpack_from('<II', data, pos)
            self.chunk_lengths.append(n)
            body = data[pos + 8:pos + 8 + n]
            if kind == JSON_CHUNK:
                self.doc = json.loads(body.decode())
            elif kind == BIN_CHUNK:
                self.bin = body
            pos += 8 + n

    def view(self, i):
        v = self.doc['bufferViews'][i]
        return self.bin[v.get('byteOffset', 0):v.get('byteOffset', 0) + v['byteLength']]

    def accessor(self, i):
        a = self.doc['accessors'][i]
        cols = {'SCALAR': 1, 'VEC2': 2, 'VEC3': 3}[a['type']]
        arr = np.frombuffer(self.view(a['bufferView']), _NP[a['componentType']], a['count'] * cols,
                            a.get('byteOffset', 0))
        return arr.reshape(a['count'], cols) if cols > 1 else arr

    def node(self, name):
        return next(n for n in self.doc['nodes'] if n['name'] == name)

    def primitive(self, name):
        return self.doc['meshes'][self.node(name)['mesh']]['primitives'][0]

    def image(self, i=0):
        return png.decode(self.view(self.doc['images'][i]['bufferView']))
