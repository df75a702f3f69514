"""What tests/test_gpu_wf_head_records.py takes for granted of its scenes (tests/wf_head_records_scenes.py), on the host, no
GPU: through the hook srtTestWfHead over the CPU oracle's trees, the head word of each scene is the leaf word of the ground
(primitive 40) and of the intended second sphere (primitive 41), or of the ground alone; and the spheres of the leaf move
as the scene's name says."""
import regroup_elide as E
import wf_head_records_scenes as R
import wf_head_scenes as S
from test_wf_head_host import _first_kept, _oracle_tree


def test_head_words(oracle, abi, dev):
    pair = E.leaf_word(S.device_ref(40, 1), S.device_ref(41, 1))
    alone = E.leaf_word(S.device_ref(40, 1), S.device_ref(40, 1))
    assert pair != 0 and alone != 0 and alone & 0xffff0000 == 0x80000000
    for make, want in ((R.moving_ground_and_still, pair), (R.both_moving, pair), (R.moving_ground_alone, alone), (S.ground_and_moving, pair)):
        sb = make(abi)
        kinds = S.kinds_of(abi, sb)
        assert kinds[40:].all() and not kinds[:40].any()
        rg = _oracle_tree(oracle, dev, sb)
        assert S.head_host(dev, rg, [0], kinds) == (1, want), make.__name__
        # the first kept record is that leaf, and its hit and miss words lead to the same successor
        first, hit, _ = _first_kept(dev, rg)
        refs = rg.view("int32")[first]
        assert hit < 0 and (~int(refs[3]), ~int(refs[7])) == ((40, 41) if want == pair else (40, 40)), make.__name__


def test_which_spheres_move(abi):
    for make, moves in ((R.moving_ground_and_still, (True, False)), (R.both_moving, (True, True)), (S.ground_and_moving, (False, True)),
                        (R.moving_ground_alone, (True,) + (False,) * 7)):
        sb = make(abi)
        assert tuple(tuple(s.center0) != tuple(s.center1) for s in sb.spheres) == moves, make.__name__
        rec = R.sphere_records(abi, sb, {0: {"radius": 7.0}})
        assert len(rec) == len(moves) and float(rec[0][4]) == 7.0 and float(rec[-1][4]) == float(sb.spheres[-1].radius)
