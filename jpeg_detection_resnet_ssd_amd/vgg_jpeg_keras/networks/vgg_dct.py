"""The VGG-DCT classifiers `vgga_dct` / `vggd_dct` (classification_part/vgg_jpeg_keras/networks/networks_dct.py; the
configurations classification_part/config/vggA_dct and config/vggD_dct train them): a VGG cut down to its last two
convolution blocks, fed with the luma DCT planes at 28x28x64 and the chroma planes at 14x14x128 that
DCTGeneratorJPEG2DCT emits.  Layer names are the reference's, so load_weights(by_name=True) matches its checkpoints.

Both are one topology, `vgg_dct`, with two or three 3x3 convolutions per block; its keyword arguments let tests build
the same graph small."""
from ...keras.layers import (BatchNormalization, Concatenate, Conv2D, Dense, Dropout, Flatten, Input, MaxPooling2D)
from ...keras.models import Model


def vgg_dct(classes=1000, convs_per_block=2, filters=(256, 512, 512), fc_units=4096, input_size=28, y_channels=64,
            cbcr_channels=128, dropout_rate=0.5, name="vgg_dct"):
    """filters = (luma stem, block 4, block 5).  `input_size` is the side of the luma planes and must be a multiple of 4;
    the chroma planes have half of it."""
    if input_size % 4:
        raise ValueError("input_size must be a multiple of 4 (two 2x2 pools, chroma at half size), got %r" % (input_size,))
    stem, wide4, wide5 = filters
    input_y = Input((input_size, input_size, y_channels))
    input_cbcr = Input((input_size // 2, input_size // 2, cbcr_channels))

    x = BatchNormalization(name="b_norm_64")(input_y)
    norm_cbcr = BatchNormalization(name="b_norm_128")(input_cbcr)
    x = Conv2D(stem, (3, 3), activation="relu", padding="same", name="conv1_1_dct_256")(x)

    for i in range(convs_per_block):
        x = Conv2D(wide4, (3, 3), activation="relu", padding="same", name="conv4_%d" % (i + 1))(x)
    x = MaxPooling2D((2, 2), strides=(2, 2), name="pool4")(x)

    x = Concatenate(axis=-1)([x, norm_cbcr])
    for i in range(convs_per_block):
        x = Conv2D(wide5, (3, 3), activation="relu", padding="same", name="conv5_%d" % (i + 1))(x)
    x = MaxPooling2D((2, 2), strides=(2, 2), name="pool5")(x)

    x = Flatten(name="flatten")(x)
    x = Dense(fc_units, activation="relu", name="fc1")(x)
    x = Dropout(dropout_rate)(x)
    x = Dense(fc_units, activation="relu", name="fc2")(x)
    x = Dropout(dropout_rate)(x)
    x = Dense(classes, activation="softmax", name="predictions")(x)
    return Model(inputs=[input_y, input_cbcr], outputs=x, name=name)


def vgga_dct(classes=1000):
    """VGG-A in the DCT domain: two convolutions per block."""
    return vgg_dct(classes, convs_per_block=2, name="vgga_dct")


def vggd_dct(classes=1000):
    """VGG-D in the DCT domain: three convolutions per block."""
    return vgg_dct(classes, convs_per_block=3, name="vggd_dct")
