"""Sequential restatement of the COCO mask API's rleEncode, rleArea and rleToBbox (maskApi.c), the specification of
ep24.cocomask.encode and of the records ep24.results writes.  Plain Python, one statement per step of the C code; the string
forms and the decoder are tests/cocomask_oracle.py's."""
from cocomask_oracle import rle_decode, rle_from_string, rle_to_string  # noqa: F401


def rle_encode(mask):
    """rleEncode of rows of 0 / 1 (mask[y][x]): the column-major walk, previous value 0, every change closes a run."""
    h, w = len(mask), len(mask[0])
    cnts, p, c = [], 0, 0
    for j in range(h * w):
        v = 1 if mask[j % h][j // h] else 0
        if v != p:
            cnts.append(c)
            c = 0
            p = v
        c += 1
    cnts.append(c)
    return cnts


def rle_area(cnts):
    """rleArea: the sum of the odd-indexed counts."""
    return sum(cnts[1::2])


def rle_to_bbox(cnts, h, w):
    """rleToBbox: [x, y, w, h] from the runs alone; [0, 0, 0, 0] for a mask without a set pixel."""
    m = len(cnts) // 2 * 2
    if m == 0:
        return [0, 0, 0, 0]
    xs, ys, xe, ye, cc, xp = w, h, 0, 0, 0, 0
    for j in range(m):
        cc += cnts[j]
        t = cc - j % 2
        y, x = t % h, (t - t % h) // h
        if j % 2 == 0:
            xp = x
        elif xp < x:
            ys, ye = 0, h - 1
        xs, xe, ys, ye = min(xs, x), max(xe, x), min(ys, y), max(ye, y)
    return [xs, ys, xe - xs + 1, ye - ys + 1]
