"""8-bit RGB PNG files with the standard library only (zlib + struct): what the overlay entry points write in place of
torchvision.utils.save_image, which is absent here.

write() stores [H, W, 3] uint8 as colour type 2, bit depth 8, no interlace, filter type 0 on every row.  read() decodes
what write() produces and, more generally, any non-interlaced 8-bit RGB file with filter types 0-4 (e.g. Pillow's)."""
import struct
import zlib

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'


def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)


def encode(rgb, level=6):
    """PNG bytes of an [H, W, 3] uint8 array (numpy or a CPU tensor)."""
    a = np.ascontiguousarray(np.asarray(rgb))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError('png.encode wants [H, W, 3] uint8, got %s %s' % (a.dtype, a.shape))
    H, W, _ = a.shape
    raw = np.zeros((H, 1 + 3 * W), np.uint8)          # filter byte 0 (None) in front of every row
    raw[:, 1:] = a.reshape(H, 3 * W)
    ihdr = struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0)
    return SIGNATURE + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', zlib.compress(raw.tobytes(), level)) + _chunk(b'IEND', b'')


def write(path, rgb, level=6):
    with open(path, 'wb') as f:
        f.write(encode(rgb, level))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def _unfilter(data, H, W, bpp=3):
    stride = W * bpp
    out = np.zeros((H, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    pos = 0
    for y in range(H):
        ft = data[pos]
        line = np.frombuffer(data, np.uint8, stride, pos + 1).astype(np.int32)
        pos += 1 + stride
        if ft == 0:
            cur = line
        elif ft == 1:          # Sub: runs along the row, one channel at a time
            cur = line.copy()
            for c in range(bpp):
                cur[c::bpp] = np.cumsum(line[c::bpp]) & 0xff
        elif ft == 2:          # Up
            cur = (line + prev) & 0xff
        elif ft == 3:          # Average
            cur = line.copy()
            for i in range(stride):
                left = cur[i - bpp] if i >= bpp else 0
                cur[i] = (line[i] + ((left + int(prev[i])) >> 1)) & 0xff
        elif ft == 4:          # Paeth
            cur = line.copy()
            for i in range(stride):
                left = cur[i - bpp] if i >= bpp else 0
                ul = int(prev[i - bpp]) if i >= bpp else 0
                cur[i] = (line[i] + _paeth(int(left), int(prev[i]), ul)) & 0xff
        else:
            raise ValueError('png: bad filter type %d in row %d' % (ft, y))
        out[y] = cur
        prev = cur.astype(np.int32)
    return out.reshape(H, W, bpp)


def decode(buf):
    """[H, W, 3] uint8 from the bytes of an 8-bit RGB, non-interlaced PNG."""
    if buf[:8] != SIGNATURE:
        raise ValueError('png: not a PNG file')
    pos, ihdr, idat = 8, None, []
    while pos < len(buf):
        n, kind = struct.unpack('>I4s', buf[pos:pos + 8])
        data = buf[pos + 8:pos + 8 + n]
        if zlib.crc32(kind + data) & 0xffffffff != struct.unpack('>I', buf[pos + 8 + n:pos + 12 + n])[0]:
            raise ValueError('png: CRC mismatch in %r' % kind)
        pos += 12 + n
        if kind == b'IHDR':
            ihdr = struct.unpack('>IIBBBBB', data)
        elif kind == b'IDAT':
            idat.append(data)
        elif kind == b'IEND':
            break
    if ihdr is None:
        raise ValueError('png: no IHDR')
    W, H, depth, ctype, comp, filt, interlace = ihdr
    if (depth, ctype, comp, filt, interlace) != (8, 2, 0, 0, 0):
        raise ValueError('png: only 8-bit RGB without interlace is supported (IHDR %r)' % (ihdr,))
    data = zlib.decompress(b''.join(idat))
    if len(data) != H * (1 + 3 * W):
        raise ValueError('png: %d bytes of image data, expected %d' % (len(data), H * (1 + 3 * W)))
    return _unfilter(data, H, W)


def read(path):
    with open(path, 'rb') as f:
        return decode(f.read())
