"""Task-1 result files -> Task-2 result files (the reference's DOTA_devkit/results_obb2hbb.py): every
`image score x1 y1 .. x4 y4` line becomes `image score xmin ymin xmax ymax` of the quad's horizontal hull.  Host text only;
the output is byte-identical to the reference's: the score token is copied, the four numbers are `str()` of the floats, and
the last line has no newline.
"""
import argparse
import os
import shutil


def parse_args():
    parser = argparse.ArgumentParser(description='Task-1 (OBB) result files to Task-2 (HBB) result files')
    parser.add_argument('--srcpath', required=True, help='directory of the Task-1 class files')
    parser.add_argument('--dstpath', required=True, help='directory for Task2_<class>.txt (removed and recreated)')
    return parser.parse_args()


def GetFileFromThisRootDir(dir, ext=None):
    """:15-26.  Every file below `dir`; with `ext`, those whose extension (without the dot) is `in ext`."""
    allfiles = []
    for root, _, files in os.walk(dir):
        for name in files:
            path = os.path.join(root, name)
            if ext is None or os.path.splitext(path)[1][1:] in ext:
                allfiles.append(path)
    return allfiles


def custombasename(fullname):
    """:28-29."""
    return os.path.basename(os.path.splitext(fullname)[0])


def OBB2HBB(srcpath, dstpath):
    """:31-55.  `dstpath` is removed and recreated; <anything>_<class>.txt -> Task2_<class>.txt."""
    filenames = GetFileFromThisRootDir(srcpath)
    if os.path.exists(dstpath):
        shutil.rmtree(dstpath)
    os.makedirs(dstpath)
    for file in filenames:
        classname = custombasename(file).split('_')[-1]
        with open(file, 'r') as f_in:
            rows = [line.strip().split() for line in f_in.readlines()]
        out = []
        for row in rows:
            poly = [float(v) for v in row[2:]]
            xs, ys = poly[0::2], poly[1::2]
            out.append(row[0] + ' ' + row[1] + ' ' + ' '.join(map(str, [min(xs), min(ys), max(xs), max(ys)])))
        with open(os.path.join(dstpath, 'Task2_' + classname + '.txt'), 'w') as f_out:
            f_out.write('\n'.join(out))


if __name__ == '__main__':
    args = parse_args()
    OBB2HBB(args.srcpath, args.dstpath)
